// vdl_mscan_body.h -- device code of the multi-aggregate fused scans (global and dense-domain grouped form, with or without
// derived columns): included by vdl_mscan.hip for the precompiled instantiations, and handed as text to hiprtc when a plan's
// scan is specialised at run time (vdl_jit.cpp).  HIP built-ins only -- no C++ library.
#pragma once
#include "vdl_scan_desc.h"
#include "vdl_front_index.h"

#ifndef VDL_SPEC_UNROLL
#define VDL_SPEC_UNROLL                     // specialised builds: _Pragma("unroll") on the loops a descriptor drives
#endif

namespace vdl {

typedef long long ll2 __attribute__((ext_vector_type(2)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef char i8x2 __attribute__((ext_vector_type(2)));

template <int N> struct IntTag { static constexpr int value = N; };

namespace {


constexpr int kWave = 64;
constexpr int kMsBlock = 256;
#ifndef VDL_PROJ_U
#define VDL_PROJ_U 4                          // row pairs per lane and tile of the projection scan (variant builds: -DVDL_PROJ_U=2|8)
#endif
constexpr int kProjU = VDL_PROJ_U;
constexpr int kProjTile = kMsBlock * 2 * kProjU;
enum { R_SUM = 0, R_MIN = 1, R_MAX = 2 };

// The saturated difference (VC_SUBS) is compiled into the precompiled kernels always, and into a specialised translation unit only
// when its descriptor holds such a column (vdl_jit.cpp writes VDL_SAT_DIFF ahead of this text): every other unit is the code it was.
#if !defined(VDL_SAT_DIFF) && !defined(__HIPCC_RTC__)
#define VDL_SAT_DIFF 1
#endif
#if VDL_SAT_DIFF
#define VDL_IS_DIFF(k) ((k) == VC_SUB || (k) == VC_SUBS)
#else
#define VDL_IS_DIFF(k) ((k) == VC_SUB)
#endif
// The decode of a lookup image right after the lookup (derive(), the bits MsArgs::decode has among the derived columns) likewise: always
// in the precompiled kernels, in a specialised unit only when one of its descriptors holds such a lookup (vdl_jit.cpp writes
// VDL_LOOKUP_DECODE ahead of this text).  A branch on a constant that folds away was not enough: the units of Q14, Q12 and Q19 came out
// with the same instructions in another order.
#if !defined(VDL_LOOKUP_DECODE) && !defined(__HIPCC_RTC__)
#define VDL_LOOKUP_DECODE 1
#endif
#if VDL_LOOKUP_DECODE
#define VDL_TILE_DECODE(C) ((C).decode & ~(C).derived)      // (a lookup's bit: decoded where it is looked up)
#else
#define VDL_TILE_DECODE(C) ((C).decode)
#endif
__device__ __forceinline__ int rk_of(int kind) { return kind == AGG_SUM ? R_SUM : kind == AGG_MAX ? R_MAX : R_MIN; }
__device__ __forceinline__ int64_t r_identity(int rk) { return rk == R_SUM ? 0 : rk == R_MIN ? INT64_MAX : INT64_MIN; }
__device__ __forceinline__ int64_t r_combine(int rk, int64_t a, int64_t b) {
    if (rk == R_SUM) return (int64_t)((uint64_t)a + (uint64_t)b);
    if (rk == R_MIN) return a < b ? a : b;
    return a > b ? a : b;
}
__device__ __forceinline__ int64_t wave_reduce(int64_t x, int rk) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) x = r_combine(rk, x, __shfl_down(x, off, kWave));
    return x;
}
#ifdef VDL_WIDE
// WIDE SUMS (vdl_plan_set_wide_sums): every SUM accumulator is a pair (lo, hi) -- bits 0..63 and 64..127 of the
// exact two's-complement sum of the int64 terms.  lo is the word the plain build keeps; only the accumulation widens, the term stays the
// int64 the program computes.  The aggregates keep their words, the high words of the SUM aggregates lie behind them in aggregate
// order: LDS lane slots nagg .. nagg + nsum - 1 (global form), G * nsum words behind a replica's table (grouped form), and the same
// in the block's partials.  Two 64-bit adds and a compare per step: no 128-bit type, no library call.
#ifdef VDL_BATCH
#error "wide sums are not batched: a plan with the switch on runs alone (vdl_run_batch)"
#endif
__device__ __forceinline__ int wide_nsum(const MScanDesc &D, int j) {      // SUM aggregates below j: where aggregate j's high word lies
    int h = 0;
#pragma unroll
    for (int k = 0; k < kMaxGroupAggs; k++) h += (k < j && D.agg[k].kind == AGG_SUM) ? 1 : 0;
    return h;
}
__device__ __forceinline__ void wide_add(uint64_t &lo, uint64_t &hi, uint64_t blo, uint64_t bhi) {
    lo += blo;
    hi += bhi + (uint64_t)(lo < blo);
}
__device__ __forceinline__ void wide_wave_reduce(uint64_t &lo, uint64_t &hi) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const uint64_t blo = __shfl_down(lo, off, kWave), bhi = __shfl_down(hi, off, kWave);
        wide_add(lo, hi, blo, bhi);
    }
}
#endif
__device__ __forceinline__ int64_t load_scalar(const void *p, int width, int64_t i) {
    switch (width) {
    case 8: return ((const int64_t *)p)[i];
    case 4: return ((const int32_t *)p)[i];
    case 2: return ((const int16_t *)p)[i];
    default: return ((const int8_t *)p)[i];
    }
}
// Masked loads without branches.  `if (on) v = *p` makes the compiler branch around the load and wait for it inside the branch
// (vmcnt(0): every load in flight, the tile's included), so a row slice's late loads became serial round trips.  A buffer
// load through a resource of `bytes` bytes from `p` asks memory for nothing and returns 0 where its offset lies past the
// resource: a lane whose row is out passes kBufOut, and every lane's load issues in one straight line.  `p` and `bytes` must be
// wave-uniform (the resource lives in scalar registers); offsets are 32 bits, so a resource spans one tile of a column,
// whatever the size of the column.
constexpr uint32_t kBufOut = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void *p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), (short)0, (int)bytes, 0x00020000);
}
// an adjacent row pair of width W at byte offset `off` in one load, both 0 where !on
template <int W>
__device__ __forceinline__ void buf_load_pair(__amdgpu_buffer_rsrc_t rs, bool on, uint32_t off, int64_t &a, int64_t &b) {
    const int o = (int)(on ? off : kBufOut);
    if (W == 8) {
        const auto x = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0);
        a = (int64_t)(((uint64_t)x[1] << 32) | x[0]); b = (int64_t)(((uint64_t)x[3] << 32) | x[2]);
    } else if (W == 4) {
        const auto x = __builtin_amdgcn_raw_buffer_load_b64(rs, o, 0, 0);
        a = (int32_t)x[0]; b = (int32_t)x[1];
    } else if (W == 2) {
        const uint32_t x = __builtin_amdgcn_raw_buffer_load_b32(rs, o, 0, 0);
        a = (int16_t)(x & 0xffffu); b = (int16_t)(x >> 16);
    } else {
        const uint32_t x = __builtin_amdgcn_raw_buffer_load_b16(rs, o, 0, 0);
        a = (int8_t)(x & 0xffu); b = (int8_t)(x >> 8);
    }
}
// one row of width W at byte offset `off`, 0 where !on (the single-row form of buf_load_pair)
template <int W>
__device__ __forceinline__ int64_t buf_load_one(__amdgpu_buffer_rsrc_t rs, bool on, uint32_t off) {
    const int o = (int)(on ? off : kBufOut);
    if (W == 8) { const auto x = __builtin_amdgcn_raw_buffer_load_b64(rs, o, 0, 0); return (int64_t)(((uint64_t)x[1] << 32) | x[0]); }
    if (W == 4) return (int32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, o, 0, 0);
    if (W == 2) return (int16_t)__builtin_amdgcn_raw_buffer_load_b16(rs, o, 0, 0);
    return (int8_t)__builtin_amdgcn_raw_buffer_load_b8(rs, o, 0, 0);
}
// value j of a lane's bit stream of `b` bits per value (the packed images of vdl_column_image.h): j and b are compile-time
// constants in the specialised builds, so this is one bit-field extract, or an align and an extract where the value straddles
// two dwords
__device__ __forceinline__ uint32_t unpack_bits(const uint32_t (&w)[32], int j, int b) {
    const int o = j * b, k = o >> 5, sh = o & 31;
    if (b >= 32) return w[k & 31];
    if (sh + b <= 32) return __builtin_amdgcn_ubfe(w[k & 31], (unsigned)sh, (unsigned)b);
    return __builtin_amdgcn_ubfe(__builtin_amdgcn_alignbit(w[(k + 1) & 31], w[k & 31], (unsigned)sh), 0u, (unsigned)b);
}
// a value read from a column image (vdl_column_image.h) as the column holds it: base + scale * e, in wrapping 64-bit arithmetic
__device__ __forceinline__ int64_t img_decode(int64_t e, int64_t base, int64_t scale) {
    return (int64_t)((uint64_t)base + (uint64_t)scale * (uint64_t)e);
}
// Step images (vdl_column_image.h Steps): `p` = the head words, one per 64 rows, padded to whole tiles of the projection scans, the
// 32-bit anchors behind them.  Row r is base + anchor[r >> 6] + the head bits of its group up to and including its own.
__host__ __device__ inline int64_t step_groups_padded(int64_t n) { return (n + kProjTile - 1) / kProjTile * (kProjTile / 64); }
__device__ __forceinline__ const uint32_t *step_anchors(const void *p, int64_t n) { return (const uint32_t *)((const uint64_t *)p + step_groups_padded(n)); }
// `w` is the width the binder gives the column: 4 when every value of the image fits 32 signed bits (base .. base + n - 1 does) -- the
// sum is then made in 32 bits and the compiler knows the upper half, as it does of a 4-byte load -- else 8.
__device__ __forceinline__ int64_t step_sum(int64_t base, uint32_t anchor, uint64_t masked, int w) {
    if (w <= 4) return (int64_t)(int32_t)((uint32_t)base + anchor + (uint32_t)__popcll(masked));
    return (int64_t)((uint64_t)base + (uint64_t)anchor + (uint64_t)__popcll(masked));
}
// one row anywhere (a survivor of the take side): two loads
__device__ __forceinline__ int64_t step_load(const void *p, int64_t n, int64_t base, int w, int64_t r) {
    return step_sum(base, step_anchors(p, n)[r >> 6], ((const uint64_t *)p)[r >> 6] & (~0ull >> (63 - (int)(r & 63))), w);
}
// A lane's rows of a tile, (base + u * 2 * kMsBlock, + 1) for u < U with base even: a pair lies in one group -- its head word and its
// anchor, the same address for the 32 lanes of half a wave (24 bytes per wave and row slice where a 4-byte column asks for 512) --
// and a population count per row gives both values.  The sub-iterations start a whole number of groups apart: one address each
// for the words and the anchors, the rest immediate offsets, and one pair of masks for all of them.  Every load goes out before
// the first count.  The partial last tile takes this path too: the image is padded to whole tiles, rows past n decode to row n - 1.
template <int U>
__device__ __forceinline__ void step_tile(const void *p, int64_t n, int64_t base, int64_t sb, int w, int64_t (&v)[2 * U]) {
    static_assert((kMsBlock * 2) % 64 == 0, "a tile's sub-iterations start whole groups apart");
    constexpr int GU = kMsBlock * 2 / 64;
    const uint64_t *hp = (const uint64_t *)p + (base >> 6);
    const uint32_t *ap = step_anchors(p, n) + (base >> 6);
    uint64_t h[U];
    uint32_t a[U];
#pragma unroll
    for (int u = 0; u < U; u++) { h[u] = hp[u * GU]; a[u] = ap[u * GU]; }
    const int i = (int)(base & 63);
    const uint64_t m0 = ~0ull >> (63 - i), m1 = ~0ull >> (62 - i);
#pragma unroll
    for (int u = 0; u < U; u++) {
        v[2 * u] = step_sum(sb, a[u], h[u] & m0, w);
        v[2 * u + 1] = step_sum(sb, a[u], h[u] & m1, w);
    }
}
template <bool NT, typename V>
__device__ __forceinline__ V stream_load(const char *p) {
    if (NT) return __builtin_nontemporal_load((const V *)p);
    return *(const V *)p;
}

// key-program operators: apply_bin minus Divide / Modulo (the planner keeps those off this path)
__device__ __forceinline__ int64_t key_bin(int op, int64_t a, int64_t b) {
    switch (op) {
    case B_LAND: return (a != 0) && (b != 0);
    case B_LOR:  return (a != 0) || (b != 0);
    case B_BAND: return a & b;
    case B_BOR:  return a | b;
    case B_SHIFT:
        if (b >= 0) return a >> (b > 63 ? 63 : b);
        if (b <= -64) return 0;
        return (int64_t)((uint64_t)a << (unsigned)(-b));
    case B_EQ:  return a == b;
    case B_ADD: return (int64_t)((uint64_t)a + (uint64_t)b);
    case B_SUB: return (int64_t)((uint64_t)a - (uint64_t)b);
    case B_GT:  return a > b;
    default:    return (int64_t)((uint64_t)a * (uint64_t)b);
    }
}

// x[r] = x[r] op k (or k op x[r]) for all rows; the operator switch is wave-uniform and sits OUTSIDE
// the row loop (a per-row switch made the kernel scalar-issue bound)
#define VDL_ROWS(EXPR) { _Pragma("unroll") for (int r = 0; r < RW; r++) { const int64_t a = x[r]; x[r] = (EXPR); } }
template <int RW>
__device__ __forceinline__ void key_rows(int op, int const_left, int64_t (&x)[RW], int64_t k) {
    switch (op) {
    case B_BAND: VDL_ROWS(a & k) break;
    case B_BOR:  VDL_ROWS(a | k) break;
    case B_ADD:  VDL_ROWS((int64_t)((uint64_t)a + (uint64_t)k)) break;
    case B_MUL:  VDL_ROWS((int64_t)((uint64_t)a * (uint64_t)k)) break;
    case B_SUB:  if (const_left) VDL_ROWS((int64_t)((uint64_t)k - (uint64_t)a)) else VDL_ROWS((int64_t)((uint64_t)a - (uint64_t)k)) break;
    case B_SHIFT:
        if (const_left) VDL_ROWS(key_bin(B_SHIFT, k, a))
        else if (k >= 0) { const int sh = k > 63 ? 63 : (int)k; VDL_ROWS(a >> sh) }
        else if (k <= -64) VDL_ROWS(0 * a)
        else { const int sh = (int)(-k); VDL_ROWS((int64_t)((uint64_t)a << sh)) }
        break;
    default:
        if (const_left) VDL_ROWS(key_bin(op, k, a)) else VDL_ROWS(key_bin(op, a, k))
        break;
    }
}
#undef VDL_ROWS
template <int RW>
__device__ __forceinline__ void key_combine(int op, int swap, int64_t (&acc)[RW], const int64_t (&tmp)[RW]) {
    switch (op) {
    case B_BOR:
#pragma unroll
        for (int r = 0; r < RW; r++) acc[r] |= tmp[r];
        break;
    case B_BAND:
#pragma unroll
        for (int r = 0; r < RW; r++) acc[r] &= tmp[r];
        break;
    case B_ADD:
#pragma unroll
        for (int r = 0; r < RW; r++) acc[r] = (int64_t)((uint64_t)acc[r] + (uint64_t)tmp[r]);
        break;
    default:
#pragma unroll
        for (int r = 0; r < RW; r++) acc[r] = swap ? key_bin(op, tmp[r], acc[r]) : key_bin(op, acc[r], tmp[r]);
        break;
    }
}


// (sbase: the bases of the columns of C.steps, MScanDesc::ibase -- the projection scans pass it; aggregate scans bind no step image)
template <int NC, int U, bool VEC, bool NT>
__device__ __forceinline__ void load_tile(const MsArgs &C, const MsArgs &Cr, int64_t base, int64_t (&v)[NC][2 * U], uint32_t skip = 0, const int64_t *sbase = nullptr) {
    constexpr int BS = kMsBlock;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        if (c < C.ncol && !(((C.derived | skip) >> c) & 1u)) {      // wave-uniform
            const char *p = (const char *)Cr.ptr[c];
            const int w = C.width(c);
            if (sbase && ((C.steps >> c) & 1u)) {                   // wave-uniform
                step_tile<U>(p, Cr.n, base, sbase[c], w, v[c]);
            } else if (!VEC) {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    v[c][2 * u] = load_scalar(p, w, base + (int64_t)u * (BS * 2));
                    v[c][2 * u + 1] = load_scalar(p, w, base + (int64_t)u * (BS * 2) + 1);
                }
            } else if (w == 8) {
#pragma unroll
                for (int u = 0; u < U; u++) { ll2 x = stream_load<NT, ll2>(p + (base + (int64_t)u * (BS * 2)) * 8); v[c][2 * u] = x.x; v[c][2 * u + 1] = x.y; }
            } else if (w == 4) {
#pragma unroll
                for (int u = 0; u < U; u++) { i32x2 x = stream_load<NT, i32x2>(p + (base + (int64_t)u * (BS * 2)) * 4); v[c][2 * u] = x.x; v[c][2 * u + 1] = x.y; }
            } else if (w == 2) {
#pragma unroll
                for (int u = 0; u < U; u++) { i16x2 x = stream_load<NT, i16x2>(p + (base + (int64_t)u * (BS * 2)) * 2); v[c][2 * u] = x.x; v[c][2 * u + 1] = x.y; }
            } else {
#pragma unroll
                for (int u = 0; u < U; u++) { i8x2 x = stream_load<NT, i8x2>(p + (base + (int64_t)u * (BS * 2))); v[c][2 * u] = x.x; v[c][2 * u + 1] = x.y; }
            }
        }
    }
}

// The select side of a projection scan: the columns of C.decode -- read from an image of scale 1 (vdl_column_image.h usable_in_vscan)
// because their values are needed per row: the source of a lookup or a difference, a semi-join position, a carried value -- become
// the column's own values as soon as the tile is in, by one add (their filters were left as the plan has them); every other column
// read from an image stays in the encoded domain, its filters and formula tests rewritten by the host.
template <int NC, int RW>
__device__ __forceinline__ void decode_tile(const MsArgs &C, const MScanDesc &D, int64_t (&v)[NC][RW]) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
        if ((VDL_TILE_DECODE(C) >> c) & 1u) {               // wave-uniform
            const uint64_t ib = (uint64_t)D.ibase[c];
#pragma unroll
            for (int r = 0; r < RW; r++) v[c][r] = (int64_t)((uint64_t)v[c][r] + ib);
        }
    }
}

// The bounds of one range filter or formula test.  (clo, chi) are the descriptor's the code was built for, (rlo, rhi) the same
// pair of the launch's descriptor in device memory.  The precompiled kernels pass one object for both, a specialised build holds
// the plan's values as constants.  A specialised build with run-time bounds (VDL_RT_BOUNDS, vdl_jit.cpp) keeps only the SHAPE of
// the range as constants -- INT64_MIN: no lower bound, INT64_MAX: no upper bound, (0, 0): a point, one equality compare; any other
// pair: a bound to read -- and takes the values from the launch's descriptor by scalar loads, so that plans which differ in
// their literals alone share one kernel.  An open side still folds away, and a load nobody uses is never issued.
// (the scan's row pipeline is a lambda with two or three call sites, inlined by the compiler's own judgement; the bound loads make
// it dearer, and a scan as large as Q12's at 2 row pairs per lane was no longer inlined -- its descriptor then does not fold, 160 KB
// of code --, so builds with run-time bounds insist)
#ifdef VDL_RT_BOUNDS
#define VDL_PROCESS_INLINE __attribute__((always_inline))
#else
#define VDL_PROCESS_INLINE
#endif
__device__ __forceinline__ void range_bounds(int64_t clo, int64_t chi, int64_t rlo, int64_t rhi, int64_t &lo, int64_t &hi) {
#ifdef VDL_RT_BOUNDS
    lo = clo == INT64_MIN ? clo : rlo;
    hi = chi == INT64_MAX ? chi : (clo == 0 && chi == 0) ? lo : rhi;
#else
    lo = clo; hi = chi;
#endif
}

template <int NC, int RW>
__device__ __forceinline__ void eval_pass(const MsArgs &C, const MScanDesc &D, const MScanDesc &Dr, const int64_t (&v)[NC][RW], bool (&pass)[RW]) {
#pragma unroll
    for (int r = 0; r < RW; r++) pass[r] = true;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        if ((C.filtered >> c) & 1u) {                      // wave-uniform (bits only below ncol)
            int64_t lo, hi;
            range_bounds(D.flo[c], D.fhi[c], Dr.flo[c], Dr.fhi[c], lo, hi);
#pragma unroll
            for (int r = 0; r < RW; r++) pass[r] = pass[r] & (v[c][r] >= lo) & (v[c][r] <= hi);
        }
    }
}

#ifdef VDL_BATCH
// eval_pass of a batched scan: it runs once per slot, so its compares are the kernel's cost (Q6 x 8: five per row and slot), and they
// are made as narrow as the column.  A closed side of a range under run-time bounds lies strictly inside the domain its column is read
// in (vdl_jit.cpp range_shape: a bound at or beyond the domain's end is an open side and folds away) or selects nothing; the bounds of
// a packed column are the packed image's, 32 unsigned bits, and those of a column or byte image of 1 or 2 bytes are handed in clamped
// to one step outside its domain (vdl_specialise.cpp batch_launch), 32 signed bits, for every slot: they have one shape.
template <int NC, int RW>
__device__ __forceinline__ void eval_pass_narrow(const MsArgs &C, const MScanDesc &D, const MScanDesc &Dr, const int64_t (&v)[NC][RW], bool (&pass)[RW], uint32_t of = ~0u) {
#pragma unroll
    for (int r = 0; r < RW; r++) pass[r] = true;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        if (((C.filtered & of) >> c) & 1u) {               // wave-uniform (bits only below ncol; `of`: the table columns of a join batch)
            int64_t lo, hi;
            range_bounds(D.flo[c], D.fhi[c], Dr.flo[c], Dr.fhi[c], lo, hi);
            if ((C.packed >> c) & 1u) {
#pragma unroll
                for (int r = 0; r < RW; r++) pass[r] = pass[r] & ((uint32_t)v[c][r] >= (uint32_t)lo) & ((uint32_t)v[c][r] <= (uint32_t)hi);
            } else if (C.width(c) < 4 && D.flo[c] != INT64_MIN && D.fhi[c] != INT64_MAX) {
#pragma unroll
                for (int r = 0; r < RW; r++) pass[r] = pass[r] & ((int32_t)v[c][r] >= (int32_t)lo) & ((int32_t)v[c][r] <= (int32_t)hi);
            } else if (C.width(c) < 4 && D.flo[c] != INT64_MIN) {
#pragma unroll
                for (int r = 0; r < RW; r++) pass[r] = pass[r] & ((int32_t)v[c][r] >= (int32_t)lo);
            } else if (C.width(c) < 4 && D.fhi[c] != INT64_MAX) {
#pragma unroll
                for (int r = 0; r < RW; r++) pass[r] = pass[r] & ((int32_t)v[c][r] <= (int32_t)hi);
            } else {
#pragma unroll
                for (int r = 0; r < RW; r++) pass[r] = pass[r] & (v[c][r] >= lo) & (v[c][r] <= hi);
            }
        }
    }
}
#endif

// Derived columns (vdl_fuse.h VColKind): values looked up through an earlier column -- the dimension side of an FK join
// seen from the fact table (Vlite.hs:1199-1282).  `alive` starts as "the direct range filters pass", so rows a cheap
// filter already rejects do no lookups (Q14 keeps 1 row in 84); a lookup out of range makes the row EPS (alive = false).
template <int NC, int RW>
__device__ __forceinline__ void derive(const MsArgs &C, const MsArgs &Cr, const MScanDesc &D, const MScanDesc &Dr, int64_t (&v)[NC][RW], bool (&alive)[RW], uint32_t only,
                                       const int64_t (&rowid)[RW] /* global row ids: Cr.row0 + index */, bool direct_filters = true) {
    if (direct_filters) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (((C.filtered >> c) & 1u) && !((C.derived >> c) & 1u)) {
                int64_t lo, hi;
                range_bounds(D.flo[c], D.fhi[c], Dr.flo[c], Dr.fhi[c], lo, hi);
#pragma unroll
                for (int r = 0; r < RW; r++) alive[r] = alive[r] & (v[c][r] >= lo) & (v[c][r] <= hi);
            }
        }
    }
    // (a row-id column has no source and may come FIRST -- the select pass of a front whose only deciding columns are the row id and
    // the set it is looked up in; every other derived column has an earlier one to derive from, so the loop starts at 1)
    if ((only & 1u) && D.dkind[0] == VC_ROWID) {
#pragma unroll
        for (int r = 0; r < RW; r++) v[0][r] = rowid[r] - Cr.rowid_base;
    }
#pragma unroll
    for (int c = 1; c < NC; c++) {
        if ((only >> c) & 1u) {                            // wave-uniform
            const int kind = D.dkind[c], a = D.dsrc[c], b = D.dsrc2[c];
            if (kind == VC_ROWID) {
#pragma unroll
                for (int r = 0; r < RW; r++) v[c][r] = rowid[r] - Cr.rowid_base;
                continue;
            }
            if (kind == VC_FORM) {
                // A boolean formula over range tests of earlier columns.  Descriptor layout (bind_forms, vdl_engine.cpp): D.dtests[c]
                // tests sorted by column -- so each column's tests run with the column index a compile-time constant, no
                // chain of selects -- then the postfix program over their result bits (REF j pushes test j), evaluated on a
                // stack of bits (bit 0 = top).  The tests of a row slice in which no lane is still alive are skipped
                // (wave-uniform; its value is never read -- for Q19, where the cheap filters and the part bitmap leave 1 row
                // in 400, that is 5 slices in 6).  An instruction budget matters here: at 8 TB/s a wave has about 140 vector
                // instructions per row slice of a 28 B/row scan.
                const int L = D.dtests[c];
                bool live[RW];
                uint64_t bits[RW];
                uint32_t stk[RW];
#pragma unroll
                for (int r = 0; r < RW; r++) { live[r] = __ballot(alive[r]) != 0; bits[r] = 0; stk[r] = 0; }
                VDL_SPEC_UNROLL
                for (int j = 0; j < L; j++) {              // (runtime loops outside, the unrolled ones inside: the column array stays in registers)
                    const int col = D.form[a + j].col;
                    int64_t lo, hi;
                    range_bounds(D.form[a + j].lo, D.form[a + j].hi, Dr.form[a + j].lo, Dr.form[a + j].hi, lo, hi);
#pragma unroll
                    for (int k = 0; k < NC; k++) {
                        if (k < c && k == col) {           // scalar branch: one body runs
#pragma unroll
                            for (int r = 0; r < RW; r++)
                                if (live[r]) bits[r] |= (uint64_t)((v[k][r] >= lo) & (v[k][r] <= hi)) << j;
                        }
                    }
                }
                VDL_SPEC_UNROLL
                for (int s = a + L; s < a + b; s++) {
                    const int op = D.form[s].op;
                    if (op == FormStep::REF) {
                        const int j = D.form[s].col;
#pragma unroll
                        for (int r = 0; r < RW; r++) stk[r] = (stk[r] << 1) | (uint32_t)((bits[r] >> j) & 1ull);
                    } else if (op == FormStep::AND) {
#pragma unroll
                        for (int r = 0; r < RW; r++) stk[r] = ((stk[r] >> 1) & ~1u) | (stk[r] & (stk[r] >> 1) & 1u);
                    } else if (op == FormStep::OR) {
#pragma unroll
                        for (int r = 0; r < RW; r++) stk[r] = (stk[r] >> 1) | (stk[r] & 1u);
                    } else if (op == FormStep::NOT) {
#pragma unroll
                        for (int r = 0; r < RW; r++) stk[r] ^= 1u;
                    } else {
#pragma unroll
                        for (int r = 0; r < RW; r++) stk[r] = (stk[r] << 1) | (op == FormStep::TRUE_ ? 1u : 0u);
                    }
                }
#pragma unroll
                for (int r = 0; r < RW; r++) v[c][r] = (int64_t)(stk[r] & 1u);
                if ((C.filtered >> c) & 1u) {
                    int64_t lo, hi;
                    range_bounds(D.flo[c], D.fhi[c], Dr.flo[c], Dr.fhi[c], lo, hi);
#pragma unroll
                    for (int r = 0; r < RW; r++) alive[r] = alive[r] & (v[c][r] >= lo) & (v[c][r] <= hi);
                }
                continue;
            }
            int64_t x[RW], y[RW];
#pragma unroll
            for (int r = 0; r < RW; r++) { x[r] = 0; y[r] = 0; }
#pragma unroll
            for (int k = 0; k < NC; k++) {                 // register files are not indexable: select the source column by comparison
                if (k < c && k == a) {
#pragma unroll
                    for (int r = 0; r < RW; r++) x[r] = v[k][r];
                }
                if (k < c && k == b) {
#pragma unroll
                    for (int r = 0; r < RW; r++) y[r] = v[k][r];
                }
            }
            if (VDL_IS_DIFF(kind)) {
#pragma unroll
                for (int r = 0; r < RW; r++) v[c][r] = (int64_t)((uint64_t)x[r] - (uint64_t)y[r]);
#if VDL_SAT_DIFF
                // VC_SUBS: where the exact difference lies outside int64 (the operands' signs differ and the result's is not x's), its
                // nearer end -- so that its sign and its zero are the exact difference's
                if (kind == VC_SUBS) {
#pragma unroll
                    for (int r = 0; r < RW; r++) if (((x[r] ^ y[r]) & (x[r] ^ v[c][r])) < 0) v[c][r] = x[r] < 0 ? INT64_MIN : INT64_MAX;
                }
#endif
                if ((C.filtered >> c) & 1u) {               // (the projection scan has no second look at the filters: fold it here)
                    int64_t lo, hi;
                    range_bounds(D.flo[c], D.fhi[c], Dr.flo[c], Dr.fhi[c], lo, hi);
#pragma unroll
                    for (int r = 0; r < RW; r++) alive[r] = alive[r] & (v[c][r] >= lo) & (v[c][r] <= hi);
                }
                continue;
            }
            const int64_t n = Dr.dn[c];
            const char *t = (const char *)Cr.ptr[c];
            const int w = C.width(c);
            bool in[RW];
#pragma unroll
            for (int r = 0; r < RW; r++) in[r] = alive[r] & (x[r] >= 0) & (x[r] < n);
            // lookups only for the lanes whose row is still alive (a selective fact filter ahead of the join -- Q14 keeps 1 row
            // in 84 -- leaves most lanes without a memory request); all the loads of a column's rows are issued before any is used
            if (kind == VC_GATHER) {
                int64_t q[RW];
#pragma unroll
                for (int r = 0; r < RW; r++) { q[r] = 0; if (in[r]) q[r] = load_scalar(t, w, x[r]); }
                // a lookup image (the byte image of the target column, vdl_column_image.h) whose values the scan needs as the column
                // holds them -- the source of a further lookup or of a difference, a semi-join position, anything the take side of a
                // front loads: decoded here, once the loads are out; every other lookup image stays encoded, its bounds rewritten
#if VDL_LOOKUP_DECODE
                if ((C.decode >> c) & 1u) {                 // wave-uniform
#pragma unroll
                    for (int r = 0; r < RW; r++) if (in[r]) q[r] = img_decode(q[r], D.ibase[c], D.iscale[c]);
                }
#endif
#pragma unroll
                for (int r = 0; r < RW; r++) { v[c][r] = q[r]; alive[r] = in[r]; }
            } else if (kind == VC_BITS) {
                uint64_t word[RW];
#pragma unroll
                for (int r = 0; r < RW; r++) word[r] = ~0ull;                      // no bitmap: every dimension row is selected
                if (t && n > 0) {                               // (unconditional: rows that are out read word 0; the bitmap is small and cached, and the loads go out together)
#pragma unroll
                    for (int r = 0; r < RW; r++) word[r] = ((const uint64_t *)t)[(in[r] ? x[r] : 0) >> 6];
                }
#pragma unroll
                for (int r = 0; r < RW; r++) { v[c][r] = in[r] ? (int64_t)((word[r] >> (x[r] & 63)) & 1ull) : 0; alive[r] = in[r]; }
            } else if (kind == VC_LUT) {                    // outside the table: 0, not EPS (Like over an offset outside the heap)
#pragma unroll
                for (int r = 0; r < RW; r++) { v[c][r] = 0; if (in[r]) v[c][r] = ((const int64_t *)t)[x[r]]; }
            } else {                                        // VC_INRANGE
#pragma unroll
                for (int r = 0; r < RW; r++) { v[c][r] = 1; alive[r] = in[r]; }
            }
            // a filter on the looked-up value (the dimension selection's bit, a dimension column's range) takes effect at
            // once: the lookups of the columns after it are then issued for the rows that are still in
            if ((C.filtered >> c) & 1u) {
                int64_t lo, hi;
                range_bounds(D.flo[c], D.fhi[c], Dr.flo[c], Dr.fhi[c], lo, hi);
#pragma unroll
                for (int r = 0; r < RW; r++) alive[r] = alive[r] & (v[c][r] >= lo) & (v[c][r] <= hi);
            }
        }
    }
}

#ifdef VDL_BATCH
// A filtered derived column of a join batch (vdl_set_batch_joins): slot q keeps its bit of m[r] while the value lies inside ITS bounds
// (B.d[q]: scalar loads), in 64 bits -- a looked-up value, a difference, a bit or a condition has no narrow domain.
template <int RW, int KB>
__device__ __forceinline__ void batch_fold(const MScanDesc &D, const MsBatch &B, int c, const int64_t (&x)[RW], int (&m)[RW]) {
#pragma unroll
    for (int q = 0; q < KB; q++) {
        int64_t lo, hi;
        range_bounds(D.flo[c], D.fhi[c], B.d[q]->flo[c], B.d[q]->fhi[c], lo, hi);
#pragma unroll
        for (int r = 0; r < RW; r++) m[r] &= ~((int)!((x[r] >= lo) & (x[r] <= hi)) << q);
    }
}
// derive() for the K plans of a join batch.  What derive() keeps in `alive` is two things here: valid[r] -- the row is inside the table
// and every lookup so far was in range, which no slot's bounds decide -- and m[r], bit q set while slot q's filters have all held (on
// entry: the filters on table columns).  A row is looked up while it is valid and SOME slot still wants it; every value is computed once;
// a filter on a derived column narrows each slot's bit at once, so the lookups after it go out for the rows some slot still wants.
// Lookup tables, their sizes and the conditions' tests are the same for every slot (the host batches only such plans) and are read
// from slot 0's descriptor (Dr).
template <int NC, int RW, int KB>
__device__ __forceinline__ void derive_batch(const MsArgs &C, const MsArgs &Cr, const MScanDesc &D, const MScanDesc &Dr, const MsBatch &B, int64_t (&v)[NC][RW],
                                             bool (&valid)[RW], int (&m)[RW], uint32_t only, const int64_t (&rowid)[RW]) {
    if ((only & 1u) && D.dkind[0] == VC_ROWID) {
#pragma unroll
        for (int r = 0; r < RW; r++) v[0][r] = rowid[r] - Cr.rowid_base;
    }
#pragma unroll
    for (int c = 1; c < NC; c++) {
        if ((only >> c) & 1u) {                            // wave-uniform
            const int kind = D.dkind[c], a = D.dsrc[c], b = D.dsrc2[c];
            if (kind == VC_ROWID) {
#pragma unroll
                for (int r = 0; r < RW; r++) v[c][r] = rowid[r] - Cr.rowid_base;
            } else if (kind == VC_FORM) {
                // (the tests and the program as in derive(); a slice no slot wants any row of is skipped)
                const int L = D.dtests[c];
                bool live[RW];
                uint64_t bits[RW];
                uint32_t stk[RW];
#pragma unroll
                for (int r = 0; r < RW; r++) { live[r] = __ballot(valid[r] & (m[r] != 0)) != 0; bits[r] = 0; stk[r] = 0; }
                VDL_SPEC_UNROLL
                for (int j = 0; j < L; j++) {
                    const int col = D.form[a + j].col;
                    int64_t lo, hi;
                    range_bounds(D.form[a + j].lo, D.form[a + j].hi, Dr.form[a + j].lo, Dr.form[a + j].hi, lo, hi);
#pragma unroll
                    for (int k = 0; k < NC; k++) {
                        if (k < c && k == col) {           // scalar branch: one body runs
#pragma unroll
                            for (int r = 0; r < RW; r++)
                                if (live[r]) bits[r] |= (uint64_t)((v[k][r] >= lo) & (v[k][r] <= hi)) << j;
                        }
                    }
                }
                VDL_SPEC_UNROLL
                for (int s = a + L; s < a + b; s++) {
                    const int op = D.form[s].op;
                    if (op == FormStep::REF) {
                        const int j = D.form[s].col;
#pragma unroll
                        for (int r = 0; r < RW; r++) stk[r] = (stk[r] << 1) | (uint32_t)((bits[r] >> j) & 1ull);
                    } else if (op == FormStep::AND) {
#pragma unroll
                        for (int r = 0; r < RW; r++) stk[r] = ((stk[r] >> 1) & ~1u) | (stk[r] & (stk[r] >> 1) & 1u);
                    } else if (op == FormStep::OR) {
#pragma unroll
                        for (int r = 0; r < RW; r++) stk[r] = (stk[r] >> 1) | (stk[r] & 1u);
                    } else if (op == FormStep::NOT) {
#pragma unroll
                        for (int r = 0; r < RW; r++) stk[r] ^= 1u;
                    } else {
#pragma unroll
                        for (int r = 0; r < RW; r++) stk[r] = (stk[r] << 1) | (op == FormStep::TRUE_ ? 1u : 0u);
                    }
                }
#pragma unroll
                for (int r = 0; r < RW; r++) v[c][r] = (int64_t)(stk[r] & 1u);
            } else {
            int64_t x[RW], y[RW];
#pragma unroll
            for (int r = 0; r < RW; r++) { x[r] = 0; y[r] = 0; }
#pragma unroll
            for (int k = 0; k < NC; k++) {                 // register files are not indexable: select the source column by comparison
                if (k < c && k == a) {
#pragma unroll
                    for (int r = 0; r < RW; r++) x[r] = v[k][r];
                }
                if (k < c && k == b) {
#pragma unroll
                    for (int r = 0; r < RW; r++) y[r] = v[k][r];
                }
            }
            if (VDL_IS_DIFF(kind)) {
#pragma unroll
                for (int r = 0; r < RW; r++) v[c][r] = (int64_t)((uint64_t)x[r] - (uint64_t)y[r]);
#if VDL_SAT_DIFF
                if (kind == VC_SUBS) {
#pragma unroll
                    for (int r = 0; r < RW; r++) if (((x[r] ^ y[r]) & (x[r] ^ v[c][r])) < 0) v[c][r] = x[r] < 0 ? INT64_MIN : INT64_MAX;
                }
#endif
            } else {
            const int64_t n = Dr.dn[c];
            const char *t = (const char *)Cr.ptr[c];
            const int w = C.width(c);
            bool inside[RW], in[RW];
            // a memory request only for a row that is valid, that some slot still wants and whose index lies inside the table
#pragma unroll
            for (int r = 0; r < RW; r++) { inside[r] = (x[r] >= 0) & (x[r] < n); in[r] = valid[r] & (m[r] != 0) & inside[r]; }
            if (kind == VC_GATHER) {
                int64_t q[RW];
#pragma unroll
                for (int r = 0; r < RW; r++) { q[r] = 0; if (in[r]) q[r] = load_scalar(t, w, x[r]); }
#if VDL_LOOKUP_DECODE
                if ((C.decode >> c) & 1u) {                 // wave-uniform
#pragma unroll
                    for (int r = 0; r < RW; r++) if (in[r]) q[r] = img_decode(q[r], D.ibase[c], D.iscale[c]);
                }
#endif
#pragma unroll
                for (int r = 0; r < RW; r++) { v[c][r] = q[r]; valid[r] = valid[r] & inside[r]; }
            } else if (kind == VC_BITS) {
                uint64_t word[RW];
#pragma unroll
                for (int r = 0; r < RW; r++) word[r] = ~0ull;                      // no bitmap: every dimension row is selected
                if (t && n > 0) {
#pragma unroll
                    for (int r = 0; r < RW; r++) word[r] = ((const uint64_t *)t)[(in[r] ? x[r] : 0) >> 6];
                }
#pragma unroll
                for (int r = 0; r < RW; r++) { v[c][r] = in[r] ? (int64_t)((word[r] >> (x[r] & 63)) & 1ull) : 0; valid[r] = valid[r] & inside[r]; }
            } else if (kind == VC_LUT) {                    // outside the table: 0, not EPS
#pragma unroll
                for (int r = 0; r < RW; r++) { v[c][r] = 0; if (in[r]) v[c][r] = ((const int64_t *)t)[x[r]]; }
            } else {                                        // VC_INRANGE
#pragma unroll
                for (int r = 0; r < RW; r++) { v[c][r] = 1; valid[r] = valid[r] & inside[r]; }
            }
            }
            }
            // a filter on the column takes effect at once, slot by slot: the lookups of the columns after it go out for the rows some slot
            // still wants.  (ONE site for every kind: with a fold per kind the column loop outgrew what the compiler unrolls at four slots
            // and more, and the row's columns went to scratch memory)
            if ((C.filtered >> c) & 1u) batch_fold<RW, KB>(D, B, c, v[c], m);
        }
    }
}
#endif

// term of one aggregate for the lane's rows: product of affine column factors (a + s*col), a constant,
// or the row id (AGG_FIRST).  Everything read from `d` is wave-uniform (scalar loads).
template <int NC, int RW>
__device__ __forceinline__ void eval_term(const MAggDesc &d, const int64_t (&v)[NC][RW], const int64_t (&rowid)[RW], int64_t (&t)[RW]) {
    if (d.kind == AGG_FIRST) {
#pragma unroll
        for (int r = 0; r < RW; r++) t[r] = rowid[r];
        return;
    }
    const uint32_t used = d.used, plain = d.plain;
    bool first = true;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        if ((used >> c) & 1u) {                            // wave-uniform
            int64_t x[RW];
            if ((plain >> c) & 1u) {
#pragma unroll
                for (int r = 0; r < RW; r++) x[r] = v[c][r];
            } else {
                const int64_t a = d.fa[c], s = d.fs[c];
                if (s == 1) {
#pragma unroll
                    for (int r = 0; r < RW; r++) x[r] = (int64_t)((uint64_t)a + (uint64_t)v[c][r]);
                } else if (s == -1) {
#pragma unroll
                    for (int r = 0; r < RW; r++) x[r] = (int64_t)((uint64_t)a - (uint64_t)v[c][r]);
                } else {
#pragma unroll
                    for (int r = 0; r < RW; r++) x[r] = (int64_t)((uint64_t)a + (uint64_t)s * (uint64_t)v[c][r]);
                }
            }
            if (first) {
#pragma unroll
                for (int r = 0; r < RW; r++) t[r] = x[r];
            } else {
#pragma unroll
                for (int r = 0; r < RW; r++) t[r] = (int64_t)((uint64_t)t[r] * (uint64_t)x[r]);
            }
            first = false;
        }
    }
    if (first) {
        const int64_t k = d.constant;
#pragma unroll
        for (int r = 0; r < RW; r++) t[r] = k;
    }
}

// the group key of the lane's rows (vdl_fuse.h KeyStep, or its canonical composite form): what a grouped scan and a grouped batch
// (VDL_BATCH) address their tables by; everything read from D is wave-uniform
template <int NC, int RW>
__device__ __forceinline__ void group_key(const MScanDesc &D, const int64_t (&v)[NC][RW], int64_t (&acc)[RW]) {
    int64_t tmp[RW];
#pragma unroll
    for (int r = 0; r < RW; r++) { acc[r] = 0; tmp[r] = 0; }
    const int ncomp = D.ncomp;
    if (ncomp > 0) {
        // the composite key in straight-line code: no step records, no operator dispatch (interpreting Q1's nine
        // steps was a quarter of the kernel)
#pragma unroll
        for (int k = 0; k < kMaxKeyComps; k++) {
            if (k < ncomp) {                           // wave-uniform
                const KeyComp kc = D.comp[k];
                int64_t x[RW];
#pragma unroll
                for (int r = 0; r < RW; r++) x[r] = 0;
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    if (c == kc.col) {
#pragma unroll
                        for (int r = 0; r < RW; r++) x[r] = v[c][r];
                    }
                }
#pragma unroll
                for (int r = 0; r < RW; r++)
                    acc[r] |= (int64_t)(((uint64_t)(x[r] >> kc.rsh) - (uint64_t)kc.sub) << kc.lsh);
            }
        }
        if (D.key_masked) {
            const int64_t mk = D.key_mask;
#pragma unroll
            for (int r = 0; r < RW; r++) acc[r] &= mk;
        }
    } else
    VDL_SPEC_UNROLL
    for (int s = 0; s < D.nkey; s++) {
        const KeyStep st = D.key[s];               // wave-uniform
        if (st.kind == KeyStep::LOAD) {
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (c == st.col) {
                    if (st.target) {
#pragma unroll
                        for (int r = 0; r < RW; r++) tmp[r] = v[c][r];
                    } else {
#pragma unroll
                        for (int r = 0; r < RW; r++) acc[r] = v[c][r];
                    }
                }
            }
        } else if (st.kind == KeyStep::OPK) {
            if (st.target) key_rows<RW>(st.bin, st.const_left, tmp, st.k);
            else key_rows<RW>(st.bin, st.const_left, acc, st.k);
        } else {
            key_combine<RW>(st.bin, st.const_left, acc, tmp);
        }
    }
}

// LDS use: global form (1 + nagg) * 256 lane slots; grouped form replicas * (pcount * (1 + nagg) | 1) + 256 + nagg + 1 trash words
// C / D: what is known when the plan is bound (column kinds and widths, filters, key, conditions, aggregates); Cr / Dr: what
// is only known at launch (column bases, row counts, lookup-table sizes, the partials area).  The precompiled kernels pass the
// same objects for both; a kernel specialised for one plan (vdl_jit.cpp) passes compile-time constants for C and D, and the
// compiler folds every descriptor-driven branch and loop of this body away.
template <int NC, int U, bool VEC, bool NT, bool GROUPED, bool DER, bool STAGED = false>
__device__ __forceinline__ void mscan_body(const MsArgs &C, const MsArgs &Cr, const MScanDesc &D, const MScanDesc &Dr
#ifdef VDL_BATCH
                                           , const MsBatch &B
#endif
                                           ) {
    extern __shared__ int64_t lds[];
    constexpr int BS = kMsBlock, TILE = BS * 2 * U, ROWS = 2 * U;
    const int tid = threadIdx.x;
    const int nagg = D.nagg;
    const int W = nagg + 1;
    const int64_t G = D.pcount;
    const int64_t words = G * W;
#ifdef VDL_WIDE
    const int nsum = wide_nsum(D, nagg);
    const int64_t hwords = GROUPED ? G * nsum : 0;         // a replica's high words, [bucket][SUM aggregate], behind its table
    const int64_t rstride = (words + hwords) | 1;
#else
    const int64_t rstride = words | 1;                     // odd int64 stride: replicas start on different banks
#endif
    const int R = D.replicas;

    int64_t cnt = 0, oob = 0;
    int64_t *mytab = lds;
    int trash = 0;
#ifdef VDL_PACKED
    constexpr bool PACKED = true;
#else
    constexpr bool PACKED = false;
#endif
#ifdef VDL_CENSUS
    // a census build (measurement, never timed): the generated late loads count, per column, the distinct 128-byte lines they
    // ask for -- the memory side fetches whole lines (tools/ubench/fetch_calib) -- in lane 0's registers
    unsigned long long census_cnt[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) census_cnt[c] = 0;
#endif
#ifdef VDL_BATCH
    // The BATCHED form (vdl_run_batch; specialised global aggregate scans over table columns, every column read with the tile or the
    // stripe): VDL_BATCH plans share the pass.  A row's values and its aggregate terms do not depend on anybody's bounds and are
    // computed once; the filters and the accumulation run once per slot, against that slot's descriptor (B.d[q]: scalar loads), into
    // that slot's own count and accumulators -- VDL_BATCH x (1 + VDL_BATCH_NAGG) 64-bit values per lane, in registers (the host
    // caps the product at kMaxBatchWords), not in LDS lane slots: nothing is launched with dynamic LDS.
    // A JOIN batch (DER; vdl_set_batch_joins): the eager tile form of a scan with derived columns -- derive_batch() looks a row up once if
    // any slot still wants it and leaves every row's set of slots, which the accumulation below then reads in place of the filters.
    static_assert(!STAGED, "batched scans read nothing late");
#ifdef VDL_PACKED
    static_assert(!DER, "a join batch has the eager tile form alone");
#endif
    static_assert(GROUPED ? VDL_BATCH >= 2 && VDL_BATCH <= kMaxBatchGrouped
                          : VDL_BATCH >= 2 && VDL_BATCH <= kMaxBatch && VDL_BATCH * (1 + VDL_BATCH_NAGG) <= kMaxBatchWords, "the slots' accumulators fit their registers");
    constexpr int KB = VDL_BATCH, NA = VDL_BATCH_NAGG, NA1 = NA > 0 ? NA : 1;
    int64_t bcnt[KB], bacc[KB][NA1];
#pragma unroll
    for (int q = 0; q < KB; q++) {
        bcnt[q] = 0;
#pragma unroll
        for (int j = 0; j < NA; j++) bacc[q][j] = r_identity(rk_of(D.agg[j].kind));
    }
    // The GROUPED batch: a row's group and its aggregate terms do not depend on anybody's bounds either -- only the SET of slots whose
    // filters it passes does.  Every non-empty set (class m = sum of pq << q, 2^K - 1 of them) has a table of its own, laid out as the
    // unbatched grouped table, class m - 1 at m - 1 times `words` inside a replica: a row issues the 1 + nagg atomics the unbatched form
    // issues, whatever K is, and the classes are folded into the slots' tables once per block (the epilogue).  The empty class and the
    // rows outside the pivots go to the lane's trash row; the latter are counted per slot, in registers.
    constexpr int NCLS = (1 << KB) - 1;
    const int64_t bstride = ((int64_t)NCLS * words) | 1;   // a replica: odd, as rstride
    int boob[KB];
#pragma unroll
    for (int q = 0; q < KB; q++) boob[q] = 0;
    if (GROUPED) {
        for (int r = 0; r < R; r++)
            for (int64_t i = tid; i < (int64_t)NCLS * words; i += BS) {
                const int w = (int)(i % W);
                int rk = R_SUM;
#pragma unroll
                for (int j = 0; j < NA; j++) if (w == j + 1) rk = rk_of(D.agg[j].kind);
                lds[(int64_t)r * bstride + i] = r_identity(rk);
            }
        mytab = lds + (int64_t)(tid % R) * bstride;
        trash = (int)((int64_t)R * bstride + (int64_t)tid - (int64_t)(tid % R) * bstride);      // (the lanes' trash rows: as in the unbatched form)
        for (int64_t i = tid; i < BS + W; i += BS) lds[(int64_t)R * bstride + i] = 0;
        __syncthreads();
    }
#else
    if (GROUPED) {
        for (int r = 0; r < R; r++)
            for (int64_t i = tid; i < words; i += BS) {
                const int w = (int)(i % W);
                lds[(int64_t)r * rstride + i] = r_identity(w == 0 ? R_SUM : rk_of(D.agg[w - 1].kind));
            }
        mytab = lds + (int64_t)(tid % R) * rstride;
        // per-lane trash rows (W words each) live behind the replicas; offset relative to mytab
        // lane t's trash row is words [t, t + W) of the trash area: rows of neighbouring lanes overlap, but within one
        // atomic instruction every lane addresses its own word (same 1 + j for all), so there is no conflict
        trash = (int)((int64_t)R * rstride + (int64_t)tid - (int64_t)(tid % R) * rstride);
        for (int64_t i = tid; i < BS + W; i += BS) lds[(int64_t)R * rstride + i] = 0;
#ifdef VDL_WIDE
        for (int r = 0; r < R; r++)
            for (int64_t i = tid; i < hwords; i += BS) lds[(int64_t)r * rstride + words + i] = 0;
#endif
    } else {
        for (int j = 0; j < nagg; j++) lds[(int64_t)j * BS + tid] = r_identity(rk_of(D.agg[j].kind));
#ifdef VDL_WIDE
        for (int h = 0; h < nsum; h++) lds[(int64_t)(nagg + h) * BS + tid] = 0;
#endif
    }
    __syncthreads();
#endif

    // tile0, tile_rows: the first row (an index into the columns) and the rows of the tile the lane's rows lie in -- wave-uniform, the
    // generated late loads build their buffer resources from them
    auto process = [&](auto rows_tag, int64_t (&v)[NC][decltype(rows_tag)::value], const int64_t (&rowid)[decltype(rows_tag)::value], int64_t rows_left, auto staged_tag,
                       int64_t tile0, int64_t tile_rows) VDL_PROCESS_INLINE {
        constexpr int RW = decltype(rows_tag)::value;
        bool pass[RW];
        // Staged reads (STAGED: specialised builds, when the tuner found them quicker): only the most selective filter column comes
        // with the tile; each further filter column is read for the rows still in (masked 8-byte loads: a 64-byte sector
        // without a live row is never touched), then what derived columns and the group key need, and last the columns that
        // are only aggregate inputs, for the rows that passed everything.  Q6 keeps 1.9 % of its rows and moves ~13 of its
        // 28 B/row this way; Q14 (1 row in 84 passes the date filter) ~6 of 28.  Worthless when most rows pass (Q1).
        constexpr bool staged = STAGED && decltype(staged_tag)::value != 0;
        bool alive[RW];
#pragma unroll
        for (int r = 0; r < RW; r++) alive[r] = !DER || (int64_t)((r >> 1) * (BS * 2) + (r & 1)) < rows_left;
#ifdef VDL_PACKED
        // (the packed form: rows of the last stripe at or past n are out)
#pragma unroll
        for (int r = 0; r < RW; r++) alive[r] = alive[r] && rowid[r] - Cr.row0 < Cr.n;
#endif
        // (the stages arrive as generated straight-line code -- VDL_STAGED_PRE / _POST, vdl_jit.cpp: written as loops over
        // columns and stages with the stage numbers read from C, the compiler no longer folded the descriptor: 235 KB of code)
#ifdef VDL_BATCH
        // a join batch: the slots that want a row -- the filters on table columns per slot, narrowed by derive_batch(); 0 for a row that is
        // past the table's end or whose lookup fell outside its table (EPS for every slot)
        int want[RW];
        if constexpr (DER) {
#pragma unroll
            for (int r = 0; r < RW; r++) want[r] = 0;
#pragma unroll
            for (int q = 0; q < KB; q++) {
                bool pq[RW];
                eval_pass_narrow<NC, RW>(C, D, *B.d[q], v, pq, ~C.derived);
#pragma unroll
                for (int r = 0; r < RW; r++) want[r] |= (int)pq[r] << q;
            }
            derive_batch<NC, RW, KB>(C, Cr, D, Dr, B, v, alive, want, C.derived, rowid);
#pragma unroll
            for (int r = 0; r < RW; r++) want[r] = alive[r] ? want[r] : 0;
        }
        if (GROUPED) {
            int64_t acc[RW];
            group_key<NC, RW>(D, v, acc);
            int m[RW], off[RW];
#pragma unroll
            for (int r = 0; r < RW; r++) m[r] = 0;
            if constexpr (DER) {
#pragma unroll
                for (int r = 0; r < RW; r++) m[r] = want[r];
            } else
#pragma unroll
            for (int q = 0; q < KB; q++) {
                bool pq[RW];
                eval_pass_narrow<NC, RW>(C, D, *B.d[q], v, pq);
#pragma unroll
                for (int r = 0; r < RW; r++) m[r] |= (int)pq[r] << q;
            }
#pragma unroll
            for (int r = 0; r < RW; r++) {
                const int64_t b = (int64_t)((uint64_t)acc[r] - (uint64_t)D.pmin);
                const bool in = b >= 0 && b < G;
#pragma unroll
                for (int q = 0; q < KB; q++) boob[q] += (!in && ((m[r] >> q) & 1)) ? 1 : 0;
                // the class's table inside the lane's replica, or the lane's trash row (no slot wants the row, or no pivot holds it)
                off[r] = (in && m[r]) ? (m[r] - 1) * (int)words + (int)b * W : trash;
                atomicAdd((unsigned long long *)&mytab[off[r]], 1ull);
            }
            // (the loop as the unbatched form writes it, over the descriptor's own count: written over the constant NA, Q1's descriptor no
            // longer folded -- 125 KB of code, the descriptor in scratch memory -- where this form gives 10 KB)
            VDL_SPEC_UNROLL
            for (int j = 0; j < nagg; j++) {
                const int rk = rk_of(D.agg[j].kind);
                int64_t t[RW];
                eval_term<NC, RW>(D.agg[j], v, rowid, t);
                if (rk == R_SUM) {
#pragma unroll
                    for (int r = 0; r < RW; r++) atomicAdd((unsigned long long *)&mytab[off[r] + 1 + j], (unsigned long long)t[r]);
                } else if (rk == R_MAX) {
#pragma unroll
                    for (int r = 0; r < RW; r++) atomicMax((long long *)&mytab[off[r] + 1 + j], (long long)t[r]);
                } else {
#pragma unroll
                    for (int r = 0; r < RW; r++) atomicMin((long long *)&mytab[off[r] + 1 + j], (long long)t[r]);
                }
            }
            (void)rows_left; (void)tile0; (void)tile_rows; (void)staged; (void)alive; (void)pass; (void)want;
            return;
        } else if constexpr (DER) {
            // the slots' counts (the wave's, as below), then aggregate by aggregate -- the loop over the descriptor's own count, as the
            // unbatched form writes it: a join scan's descriptor did not fold with the terms kept side by side (NA x RW values) -- the
            // term once, and every slot's rows of it into that slot's accumulator
#pragma unroll
            for (int q = 0; q < KB; q++) {
                int here = 0;
#pragma unroll
                for (int r = 0; r < RW; r++) here += __popcll(__ballot((want[r] >> q) & 1));
                bcnt[q] += here;
            }
            VDL_SPEC_UNROLL
            for (int j = 0; j < nagg; j++) {
                const int rk = rk_of(D.agg[j].kind);
                int64_t t[RW];
                eval_term<NC, RW>(D.agg[j], v, rowid, t);
#pragma unroll
                for (int q = 0; q < KB; q++) {
                    int64_t s = r_identity(rk);
                    if (rk == R_SUM) {
#pragma unroll
                        for (int r = 0; r < RW; r++) s = (int64_t)((uint64_t)s + (uint64_t)(((want[r] >> q) & 1) ? t[r] : 0));
                    } else if (rk == R_MIN) {
#pragma unroll
                        for (int r = 0; r < RW; r++) s = (((want[r] >> q) & 1) && t[r] < s) ? t[r] : s;
                    } else {
#pragma unroll
                        for (int r = 0; r < RW; r++) s = (((want[r] >> q) & 1) && t[r] > s) ? t[r] : s;
                    }
#pragma unroll
                    for (int k = 0; k < NA; k++) if (k == j) bacc[q][k] = r_combine(rk, bacc[q][k], s);
                }
            }
            (void)rows_left; (void)tile0; (void)tile_rows; (void)staged;
            return;
        } else {
            int64_t t[NA1][RW];
#pragma unroll
            for (int j = 0; j < NA; j++) eval_term<NC, RW>(D.agg[j], v, rowid, t[j]);
#pragma unroll
            for (int q = 0; q < KB; q++) {
                bool pq[RW];
                eval_pass_narrow<NC, RW>(C, D, *B.d[q], v, pq);
                if (PACKED) {
#pragma unroll
                    for (int r = 0; r < RW; r++) pq[r] = pq[r] & alive[r];
                }
                // (the slot's count is the WAVE's: the population of each row's lane mask, scalar work -- lane 0 hands it in at the end)
                int here = 0;
#pragma unroll
                for (int r = 0; r < RW; r++) here += __popcll(__ballot(pq[r]));
                bcnt[q] += here;
#pragma unroll
                for (int j = 0; j < NA; j++) {
                    const int rk = rk_of(D.agg[j].kind);
                    int64_t s = r_identity(rk);
                    if (rk == R_SUM) {
#pragma unroll
                        for (int r = 0; r < RW; r++) s = (int64_t)((uint64_t)s + (uint64_t)(pq[r] ? t[j][r] : 0));
                    } else if (rk == R_MIN) {
#pragma unroll
                        for (int r = 0; r < RW; r++) s = (pq[r] && t[j][r] < s) ? t[j][r] : s;
                    } else {
#pragma unroll
                        for (int r = 0; r < RW; r++) s = (pq[r] && t[j][r] > s) ? t[j][r] : s;
                    }
                    bacc[q][j] = r_combine(rk, bacc[q][j], s);
                }
            }
            (void)rows_left; (void)tile0; (void)tile_rows; (void)staged; (void)want;
            return;
        }
#endif
#ifdef VDL_STAGED_PRE
        if (staged) { VDL_STAGED_PRE }
#endif
        // (scans with derived columns run their last, partial tile through this same code: rows past the end were switched off
        // above -- `rows_left` counts from the lane's first row.  Staged: the filters on table columns are already in `alive`.)
        if (DER) derive<NC, RW>(C, Cr, D, Dr, v, alive, C.derived, rowid, !staged);
        if (staged) {
#pragma unroll
            for (int r = 0; r < RW; r++) pass[r] = alive[r];
#ifdef VDL_STAGED_POST
            VDL_STAGED_POST
#endif
        } else {
            eval_pass<NC, RW>(C, D, Dr, v, pass);
            if (DER || PACKED) {
#pragma unroll
                for (int r = 0; r < RW; r++) pass[r] = pass[r] & alive[r];
            }
        }
        int off[RW];
#ifdef VDL_WIDE
        int hoff[RW] = {};                                 // the bucket's high words (read only where pass[r])
#endif
        if (GROUPED) {
            int64_t acc[RW];
            group_key<NC, RW>(D, v, acc);
#pragma unroll
            for (int r = 0; r < RW; r++) {
                const int64_t b = (int64_t)((uint64_t)acc[r] - (uint64_t)D.pmin);
                const bool in = b >= 0 && b < G;
                oob += (pass[r] && !in) ? 1 : 0;
                pass[r] = pass[r] && in;
                // rows that do not count go to this lane's own trash slot with the identity: no branches
                off[r] = pass[r] ? (int)b * W : trash;         // the trash row absorbs whatever is added: no selects below
#ifdef VDL_WIDE
                hoff[r] = pass[r] ? (int)words + (int)b * nsum : 0;
#endif
                atomicAdd((unsigned long long *)&mytab[off[r]], 1ull);
            }
        } else {
#pragma unroll
            for (int r = 0; r < RW; r++) cnt += pass[r] ? 1 : 0;
        }
#ifdef VDL_WIDE
        int hs = 0;                                        // SUM aggregates so far: the place of the next one's high word
#endif
        VDL_SPEC_UNROLL
        for (int j = 0; j < nagg; j++) {                   // runtime loop: descriptors by scalar loads (specialised: unrolled)
            const MAggDesc d = D.agg[j];                   // whole descriptor into SGPRs: one scalar-load wait per aggregate
            const int rk = rk_of(d.kind);
            int64_t t[RW];
            eval_term<NC, RW>(d, v, rowid, t);
#ifdef VDL_WIDE
            if (rk == R_SUM) {
                if (GROUPED) {
                    // A RETURNING atomic add on the low word: the adds to one word are serialised, every one sees the word as its
                    // predecessors left it, so (old + t < t) is that add's own carry and the carries of all adds sum to the number of
                    // times the word wrapped -- exact however many lanes meet in one bucket.  The high word takes sign + carry, which
                    // is 0 for a non-negative term that does not carry: then there is no second atomic.  Rows that do not count have
                    // added to the lane's trash row and leave the high words alone.
#pragma unroll
                    for (int r = 0; r < RW; r++) {
                        const uint64_t x = (uint64_t)t[r];
                        const uint64_t old = atomicAdd((unsigned long long *)&mytab[off[r] + 1 + j], (unsigned long long)x);
                        const uint64_t up = (uint64_t)(t[r] >> 63) + (uint64_t)(old + x < x);
                        if (pass[r] && up) atomicAdd((unsigned long long *)&mytab[hoff[r] + hs], (unsigned long long)up);
                    }
                } else {
                    // the general per-row step, lo += t; hi += (t >> 63) + (lo < t), over the lane's rows, then into the lane's own slots
                    uint64_t slo = 0, shi = 0;
#pragma unroll
                    for (int r = 0; r < RW; r++) {
                        const int64_t x = pass[r] ? t[r] : 0;
                        slo += (uint64_t)x;
                        shi += (uint64_t)(x >> 63) + (uint64_t)(slo < (uint64_t)x);
                    }
                    uint64_t *ls = (uint64_t *)&lds[(int64_t)j * BS + tid], *hsl = (uint64_t *)&lds[(int64_t)(nagg + hs) * BS + tid];
                    uint64_t lo = *ls, hi = *hsl;
                    wide_add(lo, hi, slo, shi);
                    *ls = lo; *hsl = hi;
                }
                hs++;
                continue;
            }
#endif
            if (GROUPED) {
                if (rk == R_SUM) {
#pragma unroll
                    for (int r = 0; r < RW; r++) atomicAdd((unsigned long long *)&mytab[off[r] + 1 + j], (unsigned long long)t[r]);
                } else if (rk == R_MAX) {
#pragma unroll
                    for (int r = 0; r < RW; r++) atomicMax((long long *)&mytab[off[r] + 1 + j], (long long)t[r]);
                } else {
#pragma unroll
                    for (int r = 0; r < RW; r++) atomicMin((long long *)&mytab[off[r] + 1 + j], (long long)t[r]);
                }
            } else {
                int64_t s = r_identity(rk);
                if (rk == R_SUM) {
#pragma unroll
                    for (int r = 0; r < RW; r++) s = (int64_t)((uint64_t)s + (uint64_t)(pass[r] ? t[r] : 0));
                } else if (rk == R_MIN) {
#pragma unroll
                    for (int r = 0; r < RW; r++) s = (pass[r] && t[r] < s) ? t[r] : s;
                } else {
#pragma unroll
                    for (int r = 0; r < RW; r++) s = (pass[r] && t[r] > s) ? t[r] : s;
                }
                int64_t *slot = &lds[(int64_t)j * BS + tid];      // this lane's own slot: no atomics, no conflicts
                *slot = r_combine(rk, *slot, s);
            }
        }
    };

    const int64_t ntiles = Cr.n / TILE;
#ifdef VDL_PACKED
    // The PACKED form (specialised global aggregate scans over table columns, C.packed): the columns of C.packed are read from their
    // bit-packed images (vdl_column_image.h Packed), in lane-transposed stripes of 2048 rows -- row 2048 s + 64 j + l is value j of lane
    // l -- that the waves take in turn.  A wave issues every dword load of a stripe (`bits` per packed column, 256 contiguous bytes
    // each) before it unpacks any, then runs the stripe through process() ROWS values of its lanes at a time: the rows a wave holds
    // for one j are 64 consecutive rows, so the late loads of a column (from its byte image, one row per lane) ask for the same lines
    // as the tile forms do.  The tile loop's row pairs (2t, 2t + 1) do not match this layout: it is a loop of its own.
    if (!GROUPED && !DER && C.packed) {
        static_assert(32 % ROWS == 0, "a lane's 32 values of a stripe split into row slices");
        const int lane = tid & (kWave - 1);
        // (the stripe is wave-uniform, and the compiler is told so: its addresses and the late loads' buffer resources stay in scalar
        // registers -- derived from tid / 64 they were per-lane values, and every late load became a loop over the lanes' resources)
        const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
        const int64_t nstripes = (Cr.n + 2047) / 2048, wstride = (int64_t)gridDim.x * (BS / kWave);
        for (int64_t s = (int64_t)blockIdx.x * (BS / kWave) + wave; s < nstripes; s += wstride) {
            uint32_t pw[NC][32];
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if ((C.packed >> c) & 1u) {                    // wave-uniform
                    const int b = C.bits(c);
                    const char *p = (const char *)Cr.ptr[c] + ((s * b) * kWave + lane) * 4;
#pragma unroll
                    for (int k = 0; k < 32; k++)
                        if (k < b) pw[c][k] = stream_load<NT, uint32_t>(p + (int64_t)k * (kWave * 4));
                }
            }
            // (every load of the stripe goes out before the first value is unpacked: left to itself the scheduler moved each load down to
            // its first use, and a stripe became `bits` round trips to memory one after the other)
            __builtin_amdgcn_sched_barrier(0);
            const int64_t tile0 = s * 2048, tile_rows = Cr.n - tile0 < 2048 ? Cr.n - tile0 : 2048;
#pragma unroll
            for (int j0 = 0; j0 < 32; j0 += ROWS) {
                int64_t v[NC][ROWS], rowid[ROWS];
#pragma unroll
                for (int r = 0; r < ROWS; r++) rowid[r] = Cr.row0 + tile0 + (int64_t)(j0 + r) * kWave + lane;
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    if ((C.packed >> c) & 1u) {                // wave-uniform
#pragma unroll
                        for (int r = 0; r < ROWS; r++) v[c][r] = (int64_t)unpack_bits(pw[c], j0 + r, C.bits(c));
                    } else if (c < C.ncol && !((C.lazy >> c) & 1u)) {
                        // a column without a packed image read with the stripe: 64 consecutive rows of its byte image per load (clamped to
                        // the last row: rows past n are out anyway)
#pragma unroll
                        for (int r = 0; r < ROWS; r++) {
                            const int64_t i = rowid[r] - Cr.row0;
                            v[c][r] = load_scalar(Cr.ptr[c], C.width(c), i < Cr.n ? i : Cr.n - 1);
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < ROWS; r++) v[c][r] = 0;
                    }
                }
                process(IntTag<ROWS>{}, v, rowid, (int64_t)1 << 40, IntTag<1>{}, tile0, tile_rows);
            }
        }
    } else
#endif
#ifdef VDL_QUEUE_FILTER
    // The QUEUE form (C.queued; specialised builds whose first filter keeps a few rows in a hundred -- Q14: one month of seven years):
    // the filter column comes with the tile and is tested there; the rows still in are queued per wave (LDS ring of row numbers), and as
    // soon as a wave holds 64 of them every lane takes one and runs the whole pipeline on it -- the other columns at the row, the
    // lookups, the aggregates.  The staged forms above do the same work in the tile's row layout, where a wave has four or five lanes
    // alive per stage and as many loads in flight: three dependent stages deep they were bound by latency at 0.41 of the peak
    // (profiles/r04/q14_bound.txt).
    if (STAGED && C.queued) {
        // (a wave holds fewer than 64 rows when it pushes a tile's -- at most 64 per row slot --, and only then takes them out 64 at a
        // time: ONE call site for the pipeline below; inlined at every push it was three copies, the lambdas stopped being inlined and
        // the descriptor went to scratch memory)
        constexpr int QNEED = kWave - 1 + ROWS * kWave;
        constexpr int QCAP = QNEED <= 128 ? 128 : QNEED <= 256 ? 256 : QNEED <= 512 ? 512 : 1024;
        static_assert(QNEED <= QCAP, "the queue holds a tile's rows beside what was left");
        __shared__ int64_t queue[kMsBlock / kWave][QCAP];
        const int lane = tid & (kWave - 1), wave = tid / kWave;
        int head = 0, held = 0;                                    // wave-uniform
        const int64_t all_tiles = (Cr.n + TILE - 1) / TILE;
        for (int64_t tile = blockIdx.x;; tile += gridDim.x) {
            const bool flush = tile >= all_tiles;                  // (block-uniform) the trip after the last tile takes out what is left
            if (!flush) {
                int64_t v[NC][ROWS], rowid[ROWS];
                const int64_t base = tile * TILE + (int64_t)tid * 2;
#pragma unroll
                for (int r = 0; r < ROWS; r++) rowid[r] = Cr.row0 + base + (int64_t)(r >> 1) * (BS * 2) + (r & 1);
                if (tile < ntiles) load_tile<NC, U, VEC, NT>(C, Cr, base, v, C.lazy);
                else {                                             // the partial last tile: clamped scalar loads
#pragma unroll
                    for (int c = 0; c < NC; c++) {
                        if (c < C.ncol && !(((C.derived | C.lazy) >> c) & 1u)) {
#pragma unroll
                            for (int r = 0; r < ROWS; r++) { const int64_t i = rowid[r] - Cr.row0; v[c][r] = load_scalar(Cr.ptr[c], C.width(c), i < Cr.n ? i : Cr.n - 1); }
                        }
                    }
                }
                bool alive[ROWS];
#pragma unroll
                for (int r = 0; r < ROWS; r++) alive[r] = rowid[r] - Cr.row0 < Cr.n;
                constexpr int RW = ROWS;
                VDL_QUEUE_FILTER
#ifdef VDL_CENSUS
                // the lines the queued rows will ask for, counted here where the rows still lie in address order: a lane's two rows are
                // adjacent, the wave's lanes hold consecutive addresses (stride 2 w), so a lane is the first asker of its 128-byte line
                // when no lower lane with a row still in lies in the same line (as the staged forms' generated census does)
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    if (c < C.ncol && ((C.lazy >> c) & 1u) && !((C.derived >> c) & 1u)) {
                        const int w = C.width(c);
#pragma unroll
                        for (int u = 0; u < U; u++) {
                            const bool any = alive[2 * u] | alive[2 * u + 1];
                            const uint64_t m = __ballot(any);
                            const uint64_t a = (uint64_t)Cr.ptr[c] + (uint64_t)(rowid[2 * u] - Cr.row0) * (uint64_t)w;
                            int lo = lane - (int)((a & 127ull) / (uint64_t)(2 * w));
                            if (lo < 0) lo = 0;
                            const bool first = any && ((m >> lo) & ((1ull << (lane - lo)) - 1ull)) == 0ull;
                            const uint64_t f = __ballot(first);
                            if (lane == 0) census_cnt[c] += (unsigned long long)__popcll(f);
                        }
                    }
                }
#endif
#pragma unroll
                for (int r = 0; r < ROWS; r++) {
                    const uint64_t m = __ballot(alive[r]);
                    if (alive[r]) queue[wave][(head + held + __popcll(m & ((1ull << lane) - 1))) & (QCAP - 1)] = rowid[r];
                    held += __popcll(m);
                }
            }
            while (held >= (flush ? 1 : kWave)) {                  // every lane takes one queued row and runs the whole pipeline on it
                const int k = held < kWave ? held : kWave;
                if (lane < k) {
                    int64_t v1[NC][1], rid[1];
                    rid[0] = queue[wave][(head + lane) & (QCAP - 1)];
#pragma unroll
                    for (int c = 0; c < NC; c++) {
                        v1[c][0] = 0;
                        if (c < C.ncol && !((C.derived >> c) & 1u)) v1[c][0] = load_scalar(Cr.ptr[c], C.width(c), rid[0] - Cr.row0);
                    }
                    process(IntTag<1>{}, v1, rid, 1, IntTag<0>{}, 0, 0);
                }
                head = (head + k) & (QCAP - 1);
                held -= k;
            }
            if (flush) break;
        }
    } else
#endif
    {
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int64_t v[NC][ROWS], rowid[ROWS];
        const int64_t base = tile * TILE + (int64_t)tid * 2;
#pragma unroll
        for (int u = 0; u < U; u++) { rowid[2 * u] = Cr.row0 + base + (int64_t)u * (BS * 2); rowid[2 * u + 1] = rowid[2 * u] + 1; }
        load_tile<NC, U, VEC, NT>(C, Cr, base, v, STAGED ? C.lazy : 0u);
        process(IntTag<ROWS>{}, v, rowid, (int64_t)1 << 40, IntTag<1>{}, tile * TILE, (int64_t)TILE);
    }
    if (blockIdx.x == gridDim.x - 1 && ntiles * TILE < Cr.n) {
        if (DER) {
            // the partial tile, in the tile's own row layout with clamped scalar loads
            int64_t v[NC][ROWS], rowid[ROWS];
            const int64_t base = ntiles * TILE + (int64_t)tid * 2;
#pragma unroll
            for (int r = 0; r < ROWS; r++) rowid[r] = Cr.row0 + base + (int64_t)(r >> 1) * (BS * 2) + (r & 1);
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (c < C.ncol && !((C.derived >> c) & 1u)) {
#pragma unroll
                    for (int r = 0; r < ROWS; r++) {
                        const int64_t i = base + (int64_t)(r >> 1) * (BS * 2) + (r & 1);
                        v[c][r] = load_scalar(Cr.ptr[c], C.width(c), i < Cr.n ? i : Cr.n - 1);
                    }
                }
            }
            process(IntTag<ROWS>{}, v, rowid, Cr.n - base, IntTag<1>{}, ntiles * TILE, Cr.n - ntiles * TILE);
        } else {
            for (int64_t i = ntiles * TILE + tid; i < Cr.n; i += BS) {      // tail rows, one per lane
                int64_t v1[NC][1], rid[1];
                rid[0] = Cr.row0 + i;
#pragma unroll
                for (int c = 0; c < NC; c++)
                    if (c < C.ncol) v1[c][0] = load_scalar(Cr.ptr[c], C.width(c), i);
                process(IntTag<1>{}, v1, rid, 1, IntTag<1>{}, i, 1);
            }
        }
    }
    }
    __syncthreads();
    __shared__ int64_t red[kMsBlock / kWave];
    const int lane = tid & (kWave - 1), wave = tid / kWave;
#ifdef VDL_BATCH
    if (GROUPED) {
        // the block's partials, [slot][words + 1]: slot q's table is the fold, word by word and by the word's own reduction, over the
        // replicas and over the classes that contain q; its last word the slot's rows outside the pivots.  K unbatched grouped partials.
        int64_t *dst = B.partials + (int64_t)blockIdx.x * KB * (words + 1);
        for (int64_t i = tid; i < KB * words; i += BS) {
            const int q = (int)(i / words);
            const int64_t wi = i % words;
            const int w = (int)(wi % W);
            int rk = R_SUM;
#pragma unroll
            for (int j = 0; j < NA; j++) if (w == j + 1) rk = rk_of(D.agg[j].kind);
            int64_t x = r_identity(rk);
            for (int m = 1; m <= NCLS; m++) {
                if (!((m >> q) & 1)) continue;
                for (int r = 0; r < R; r++) x = r_combine(rk, x, lds[(int64_t)r * bstride + (int64_t)(m - 1) * words + wi]);
            }
            dst[(int64_t)q * (words + 1) + wi] = x;
        }
        // (the waves' counts meet in the trash area: every atomic into it lies before the barrier above)
        int64_t *meet = lds + (int64_t)R * bstride;
#pragma unroll
        for (int q = 0; q < KB; q++) {
            const int64_t x = wave_reduce((int64_t)boob[q], R_SUM);
            if (lane == 0) meet[wave * KB + q] = x;
        }
        __syncthreads();
        if (tid < KB) {
            int64_t x = 0;
            for (int k = 0; k < kMsBlock / kWave; k++) x += meet[k * KB + tid];
            dst[(int64_t)tid * (words + 1) + words] = x;
        }
        (void)red; (void)cnt; (void)oob; (void)rstride; (void)bcnt; (void)bacc;
        return;
    } else {
        // the block's partials, [slot][count, aggregates]: every value folded over the wave, then over the block's waves by the lane
        // that writes it
        constexpr int WB = NA + 1;
        __shared__ int64_t bred[kMsBlock / kWave][KB * WB];
#pragma unroll
        for (int q = 0; q < KB; q++) {
#pragma unroll
            for (int w = 0; w < WB; w++) {
                const int rk = w == 0 ? R_SUM : rk_of(D.agg[w > 0 ? w - 1 : 0].kind);
                const int64_t x = w == 0 ? bcnt[q] : wave_reduce(bacc[q][w > 0 ? w - 1 : 0], rk);      // (the counts are wave-uniform already)
                if (lane == 0) bred[wave][q * WB + w] = x;
            }
        }
        __syncthreads();
        if (tid < KB * WB) {
            const int w = tid % WB;
            int rk = R_SUM;
#pragma unroll
            for (int j = 0; j < NA; j++) if (w == j + 1) rk = rk_of(D.agg[j].kind);
            int64_t y = bred[0][tid];
            for (int k = 1; k < kMsBlock / kWave; k++) y = r_combine(rk, y, bred[k][tid]);
            B.partials[(int64_t)blockIdx.x * (KB * WB) + tid] = y;
        }
        (void)red; (void)cnt; (void)oob; (void)mytab; (void)trash; (void)rstride; (void)R; (void)bstride; (void)boob;
        return;
    }
#endif
#ifdef VDL_CENSUS
    if (lane == 0 && Dr.census) {
#pragma unroll
        for (int c = 0; c < NC; c++) if (census_cnt[c]) atomicAdd(&Dr.census[c], census_cnt[c]);
    }
#endif
#ifdef VDL_WIDE
    // the block's partials with the high words behind: global [1 + nagg][nsum]; grouped [pcount * (1 + nagg)][rows outside][pcount * nsum].
    // Every pair is folded with its carry: over the replicas (grouped), over the wave and the block's waves (global).
    __shared__ int64_t redh[kMsBlock / kWave];
    if (GROUPED) {
        int64_t *dst = Dr.block_partials + (int64_t)blockIdx.x * (words + 1 + hwords);
        for (int64_t i = tid; i < words; i += BS) {
            const int w = (int)(i % W);
            const int rk = w == 0 ? R_SUM : rk_of(D.agg[w - 1].kind);
            if (w > 0 && rk == R_SUM) {
                const int64_t hi_at = (i / W) * nsum + wide_nsum(D, w - 1);
                uint64_t lo = (uint64_t)lds[i], hi = (uint64_t)lds[words + hi_at];
                for (int r = 1; r < R; r++) wide_add(lo, hi, (uint64_t)lds[(int64_t)r * rstride + i], (uint64_t)lds[(int64_t)r * rstride + words + hi_at]);
                dst[i] = (int64_t)lo;
                dst[words + 1 + hi_at] = (int64_t)hi;
                continue;
            }
            int64_t x = lds[i];
            for (int r = 1; r < R; r++) x = r_combine(rk, x, lds[(int64_t)r * rstride + i]);
            dst[i] = x;
        }
        oob = wave_reduce(oob, R_SUM);
        if (lane == 0) red[wave] = oob;
        __syncthreads();
        if (tid == 0) { int64_t x = 0; for (int w = 0; w < kMsBlock / kWave; w++) x += red[w]; dst[words] = x; }
    } else {
        int64_t *dst = Dr.block_partials + (int64_t)blockIdx.x * (W + nsum);
        int hs = 0;
        for (int j = -1; j < nagg; j++) {
            const int rk = j < 0 ? R_SUM : rk_of(D.agg[j].kind);
            const bool pair = j >= 0 && rk == R_SUM;
            if (pair) {
                uint64_t lo = (uint64_t)lds[(int64_t)j * BS + tid], hi = (uint64_t)lds[(int64_t)(nagg + hs) * BS + tid];
                wide_wave_reduce(lo, hi);
                if (lane == 0) { red[wave] = (int64_t)lo; redh[wave] = (int64_t)hi; }
            } else {
                int64_t x = j < 0 ? cnt : lds[(int64_t)j * BS + tid];
                x = wave_reduce(x, rk);
                if (lane == 0) red[wave] = x;
            }
            __syncthreads();
            if (tid == 0 && pair) {
                uint64_t lo = (uint64_t)red[0], hi = (uint64_t)redh[0];
                for (int w = 1; w < kMsBlock / kWave; w++) wide_add(lo, hi, (uint64_t)red[w], (uint64_t)redh[w]);
                dst[j + 1] = (int64_t)lo;
                dst[W + hs] = (int64_t)hi;
            } else if (tid == 0) {
                int64_t y = red[0];
                for (int w = 1; w < kMsBlock / kWave; w++) y = r_combine(rk, y, red[w]);
                dst[j + 1] = y;
            }
            if (pair) hs++;
            __syncthreads();
        }
    }
#else
    if (GROUPED) {
        int64_t *dst = Dr.block_partials + (int64_t)blockIdx.x * (words + 1);
        for (int64_t i = tid; i < words; i += BS) {
            const int w = (int)(i % W);
            const int rk = w == 0 ? R_SUM : rk_of(D.agg[w - 1].kind);
            int64_t x = lds[i];
            for (int r = 1; r < R; r++) x = r_combine(rk, x, lds[(int64_t)r * rstride + i]);
            dst[i] = x;
        }
        oob = wave_reduce(oob, R_SUM);
        if (lane == 0) red[wave] = oob;
        __syncthreads();
        if (tid == 0) { int64_t x = 0; for (int w = 0; w < kMsBlock / kWave; w++) x += red[w]; dst[words] = x; }
    } else {
        int64_t *dst = Dr.block_partials + (int64_t)blockIdx.x * W;
        for (int j = -1; j < nagg; j++) {
            const int rk = j < 0 ? R_SUM : rk_of(D.agg[j].kind);
            int64_t x = j < 0 ? cnt : lds[(int64_t)j * BS + tid];
            x = wave_reduce(x, rk);
            if (lane == 0) red[wave] = x;
            __syncthreads();
            if (tid == 0) {
                int64_t y = red[0];
                for (int w = 1; w < kMsBlock / kWave; w++) y = r_combine(rk, y, red[w]);
                dst[j + 1] = y;
            }
            __syncthreads();
        }
    }
#endif
}

// ---- projection scan (ProjPlan, vdl_fuse.h) -----------------------------------------------------------------------------
// k_project_select: ONE pass over the columns that decide a row's survival (filtered columns and what they are derived from),
// leaving the selection as a BITMAP over the table's rows (a dimension scan: Q3's orders by date and by the customer's segment,
// through the customer bitmap) or setting the bits of a semi-join set.  The fused FRONT of a fact table -- the same selection,
// then the survivors' columns as packed vectors -- is project_front_body below.  (Until round 4 the front was this pass leaving
// counts and 16-bit positions per tile, a prefix sum, and a take pass with one wave per tile.)
// Row order inside a tile is (sub-iteration u, wave, lane, row of the lane's pair).
// (kProjU, kProjTile: the tile of these scans, defined at the top -- the step images are padded to it)
static_assert(kProjTile <= 65536, "positions inside a tile fit 16 bits");

template <int NC, int U, bool VEC, bool NT>
__device__ __forceinline__ void project_select_body(const MsArgs &C, const MsArgs &Cr, const MScanDesc &D, const MScanDesc &Dr) {
    constexpr int BS = kMsBlock, ROWS = 2 * U, TILE = BS * ROWS, NW = BS / kWave;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t full = Cr.n / TILE, ntiles = (Cr.n + TILE - 1) / TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int64_t v[NC][ROWS];
        const int64_t base = tile * TILE + (int64_t)tid * 2;
        if (tile < full) {
            load_tile<NC, U, VEC, NT>(C, Cr, base, v, C.lazy, D.ibase);
        } else {                                           // the partial last tile: clamped scalar loads
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (c < C.ncol && !(((C.derived | C.lazy) >> c) & 1u)) {
                    if ((C.steps >> c) & 1u) { step_tile<U>(Cr.ptr[c], Cr.n, base, D.ibase[c], C.width(c), v[c]); continue; }      // (padded to whole tiles)
#pragma unroll
                    for (int r = 0; r < ROWS; r++) {
                        const int64_t i = base + (int64_t)(r >> 1) * (BS * 2) + (r & 1);
                        v[c][r] = load_scalar(Cr.ptr[c], C.width(c), i < Cr.n ? i : Cr.n - 1);
                    }
                }
            }
        }
        decode_tile<NC, ROWS>(C, D, v);
        bool alive[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; r++) alive[r] = base + (int64_t)(r >> 1) * (BS * 2) + (r & 1) < Cr.n;
        int64_t rid[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; r++) rid[r] = Cr.row0 + base + (int64_t)(r >> 1) * (BS * 2) + (r & 1);
        derive<NC, ROWS>(C, Cr, D, Dr, v, alive, C.derived & ~C.lazy, rid);      // filters fold into `alive` as they are derived
        if (D.bitmap_only == 2) {
            // a semi-join scan: every selected row sets the bit of its index in the set (many rows share a bit: atomic OR)
            unsigned long long *set = (unsigned long long *)Dr.out_ptr[0];
            const int64_t nbits = Dr.dn[D.out_col[0]];
#pragma unroll
            for (int k = 0; k < NC; k++) {
                if (k == D.out_col[0]) {
#pragma unroll
                    for (int r = 0; r < ROWS; r++) {
                        int64_t x = v[k][r];
                        if (D.pmin > 0) x = x % D.pmin;            // the emitted `mod N` (sign of the dividend, like the element-wise operator)
                        if (alive[r] && x >= 0 && x < nbits) atomicOr(&set[x >> 6], 1ull << (x & 63));
                    }
                }
            }
            continue;
        }
        uint64_t m[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; r++) m[r] = __ballot(alive[r]);
        // the selection's bitmap over the table's rows, for whoever asks the sparse vectors for their validity: lanes 2l, 2l+1
        // of the two ballots of a sub-iteration are rows 2l, 2l+1 of the wave's 128 -- interleave them into two words
        if (Dr.out_ptr[0] && lane < 2 * U) {
            const int u = lane >> 1, half = lane & 1;
            uint64_t a = 0, b = 0;
#pragma unroll
            for (int uu = 0; uu < U; uu++) if (uu == u) { a = m[2 * uu]; b = m[2 * uu + 1]; }
            uint64_t x = half ? (a >> 32) : (a & 0xffffffffull), y = half ? (b >> 32) : (b & 0xffffffffull);
            x = (x | (x << 16)) & 0x0000ffff0000ffffull; x = (x | (x << 8)) & 0x00ff00ff00ff00ffull; x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
            x = (x | (x << 2)) & 0x3333333333333333ull; x = (x | (x << 1)) & 0x5555555555555555ull;
            y = (y | (y << 16)) & 0x0000ffff0000ffffull; y = (y | (y << 8)) & 0x00ff00ff00ff00ffull; y = (y | (y << 4)) & 0x0f0f0f0f0f0f0f0full;
            y = (y | (y << 2)) & 0x3333333333333333ull; y = (y | (y << 1)) & 0x5555555555555555ull;
            const int64_t word = (tile * TILE + (int64_t)u * (BS * 2) + (int64_t)wave * 128) / 64 + half;
            if (word < ((Cr.n + 63) >> 6)) ((uint64_t *)Dr.out_ptr[0])[word] = x | (y << 1);
        }
    }
}

// ---- the fused front in ONE pass (round 4) ---------------------------------------------------------------------------------
// k_project_select + prefix sum + host count + k_project_take as one kernel: a block takes a tile (tiles are handed out in
// starting order), runs the select pass's work on it -- deciding columns, lookups, ballots, the survivors' ranks --, PUBLISHES the
// tile's survivor count, puts the survivors' positions (and the carried columns' values) in survivor order in LDS, learns where its
// survivors go from the counts of the tiles before it, and writes the output vectors itself: every lane takes survivors
// k, k + 256, ... as the take pass's waves did.  No tile counts, no 16-bit position scratch and no carry area in memory, no
// prefix-sum launches, no second kernel; the isolated-line fetches of the survivors' columns run beside the other blocks' streams.
// Where a block's survivors go is a prefix over work that runs at the same time; as in the radix Partition (vdl_partition.hip, where
// the reasoning and the measurements are) a Fenwick tree of fan-out 16 is kept over the counts -- here over the counts of BATCHES of
// kFrontBatch tiles (below), one word per node {ready bit, count} --: a batch's prefix is the sum of at most 15 nodes per level, fetched
// by the lanes of one wave at once; the node of 16 / 256 / ... batches is made by the batch that completes them.  A batch only waits
// for batches that already run.
struct FrontLook {
    unsigned int *ticket;              // zeroed before the launch
    unsigned long long *nodes;         // front_look_words(batches) words, zeroed
    int64_t *total;                    // the survivors' number, left by the last batch (device)
    int64_t *total_host;               // ... and in pinned host memory (may be null)
};
// (which word holds which node, who publishes what and the prefix walk: vdl_front_index.h, shared with a host program)
static_assert(kFrontWave == kWave, "the prefix walk deals the nodes to the lanes of one wave");
constexpr unsigned long long kFrontReady = 1ull << 63;
__device__ __forceinline__ int64_t front_wait(const unsigned long long *p) {
    unsigned long long v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (!(v & kFrontReady)) { __builtin_amdgcn_s_sleep(2); v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    return (int64_t)(v & ~kFrontReady);
}
__device__ __forceinline__ void front_publish(unsigned long long *p, int64_t v) {
    __hip_atomic_store(p, (unsigned long long)v | kFrontReady, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A block takes kFrontBatch consecutive tiles at a time (a "batch"): selects them one after the other, collecting the survivors of all of
// them in LDS, and only then asks where they go and fetches their columns -- with one tile per take (the first form) a block
// waited 12 us per tile for the look-back and for the take's two rounds of dependent loads with a hundred of its 256 lanes busy, and the
// pass took 435 us for Q3 at SF10 against the two-pass front's 335 (profiles/r04/q3_front_one_tile_per_take.txt).
#ifndef VDL_FRONT_BATCH
#define VDL_FRONT_BATCH 4
#endif
constexpr int kFrontBatch = VDL_FRONT_BATCH;
static_assert(kFrontBatch * kProjTile <= 65536, "positions inside a batch fit 16 bits");
constexpr int kFrontCarry = 512;                           // carried values per batch and column; survivors beyond fetch the column again

template <int NCS, int NCT, int U, bool VEC, bool NT>
__device__ __forceinline__ void project_front_body(const MsArgs &Cs, const MsArgs &Csr, const MScanDesc &Ds, const MScanDesc &Dsr,
                                                   const MsArgs &Ct, const MsArgs &Ctr, const MScanDesc &Dt, const MScanDesc &Dtr, const FrontLook &lk) {
    constexpr int BS = kMsBlock, ROWS = 2 * U, TILE = BS * ROWS, NW = BS / kWave;
    static_assert(TILE == kProjTile, "one tile shape for the projection scans");
    __shared__ int wcnt[2][U][NW];                         // by tile parity: one barrier per tile
    __shared__ unsigned int s_batch;
    __shared__ long long s_off;
    __shared__ uint16_t spos[kFrontBatch * TILE];          // the survivors' positions inside the batch, in row order
    __shared__ int64_t cst[kMaxCarry][kFrontCarry];        // the carried columns' values, in survivor order
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t full = Csr.n / TILE, ntiles = (Csr.n + TILE - 1) / TILE, nbatches = (ntiles + kFrontBatch - 1) / kFrontBatch;
    int par = 0;
    for (;;) {
        if (tid == 0) s_batch = atomicAdd(lk.ticket, 1u);
        __syncthreads();
        const int64_t batch = s_batch;
        if (batch >= nbatches) break;                      // (block-uniform)
        int total = 0;                                     // survivors of the batch so far
        for (int sub = 0; sub < kFrontBatch; sub++) {
            const int64_t tile = batch * kFrontBatch + sub;
            if (tile >= ntiles) break;                     // (block-uniform)
            int64_t v[NCS][ROWS];
            const int64_t base = tile * TILE + (int64_t)tid * 2;
            if (tile < full) {
                load_tile<NCS, U, VEC, NT>(Cs, Csr, base, v, Cs.lazy, Ds.ibase);
            } else {                                       // the partial last tile: clamped scalar loads
#pragma unroll
                for (int c = 0; c < NCS; c++) {
                    if (c < Cs.ncol && !(((Cs.derived | Cs.lazy) >> c) & 1u)) {
                        if ((Cs.steps >> c) & 1u) { step_tile<U>(Csr.ptr[c], Csr.n, base, Ds.ibase[c], Cs.width(c), v[c]); continue; }      // (padded to whole tiles)
#pragma unroll
                        for (int r = 0; r < ROWS; r++) {
                            const int64_t i = base + (int64_t)(r >> 1) * (BS * 2) + (r & 1);
                            v[c][r] = load_scalar(Csr.ptr[c], Cs.width(c), i < Csr.n ? i : Csr.n - 1);
                        }
                    }
                }
            }
            decode_tile<NCS, ROWS>(Cs, Ds, v);
            bool alive[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) alive[r] = base + (int64_t)(r >> 1) * (BS * 2) + (r & 1) < Csr.n;
            int64_t rid[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) rid[r] = Csr.row0 + base + (int64_t)(r >> 1) * (BS * 2) + (r & 1);
            derive<NCS, ROWS>(Cs, Csr, Ds, Dsr, v, alive, Cs.derived & ~Cs.lazy, rid);      // filters fold into `alive` as they are derived
            uint64_t m[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) m[r] = __ballot(alive[r]);
            // the selection's bitmap over the table's rows, for whoever asks the sparse vectors for their validity: lanes 2l, 2l+1
            // of the two ballots of a sub-iteration are rows 2l, 2l+1 of the wave's 128 -- interleave them into two words
            if (Dsr.out_ptr[0] && lane < 2 * U) {
                const int u = lane >> 1, half = lane & 1;
                uint64_t a = 0, b = 0;
#pragma unroll
                for (int uu = 0; uu < U; uu++) if (uu == u) { a = m[2 * uu]; b = m[2 * uu + 1]; }
                uint64_t x = half ? (a >> 32) : (a & 0xffffffffull), y = half ? (b >> 32) : (b & 0xffffffffull);
                x = (x | (x << 16)) & 0x0000ffff0000ffffull; x = (x | (x << 8)) & 0x00ff00ff00ff00ffull; x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
                x = (x | (x << 2)) & 0x3333333333333333ull; x = (x | (x << 1)) & 0x5555555555555555ull;
                y = (y | (y << 16)) & 0x0000ffff0000ffffull; y = (y | (y << 8)) & 0x00ff00ff00ff00ffull; y = (y | (y << 4)) & 0x0f0f0f0f0f0f0f0full;
                y = (y | (y << 2)) & 0x3333333333333333ull; y = (y | (y << 1)) & 0x5555555555555555ull;
                const int64_t word = (tile * TILE + (int64_t)u * (BS * 2) + (int64_t)wave * 128) / 64 + half;
                if (word < ((Csr.n + 63) >> 6)) ((uint64_t *)Dsr.out_ptr[0])[word] = x | (y << 1);
            }
            if (lane == 0) {
#pragma unroll
                for (int u = 0; u < U; u++) wcnt[par][u][wave] = __popcll(m[2 * u]) + __popcll(m[2 * u + 1]);
            }
            __syncthreads();
            int here = 0, mybase[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
#pragma unroll
                for (int w = 0; w < NW; w++) { if (w == wave) mybase[u] = total + here; here += wcnt[par][u][w]; }
            }
            par ^= 1;                                      // (no second barrier: the next tile's counts go to the other half)
            const uint64_t below = (1ull << lane) - 1;
            int rank[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const int u = r >> 1;
                rank[r] = mybase[u] + __popcll(m[2 * u] & below) + __popcll(m[2 * u + 1] & below) + ((r & 1) && alive[2 * u] ? 1 : 0);
                if (alive[r]) spos[rank[r]] = (uint16_t)(sub * TILE + tid * 2 + u * (BS * 2) + (r & 1));
            }
            if (Ds.carry) {
                // the survivors' values of the deciding columns that the outputs want too (the join index of a fact table whose dimension
                // is filtered): they are in registers here -- kept in survivor order instead of being fetched again line by isolated line
                // (a column read from an image is carried only when the select side holds its own values: plain or decoded with the tile)
                int ci = 0;
#pragma unroll
                for (int c = 0; c < NCS; c++) {
                    if ((Ds.carry >> c) & 1u) {
#pragma unroll
                        for (int r = 0; r < ROWS; r++) if (alive[r] && rank[r] < kFrontCarry) cst[ci][rank[r]] = v[c][r];
                        ci++;
                    }
                }
            }
            total += here;
        }
        // the batch's count goes out (every later batch needs it); a batch that completes 16 / 256 / ... also sums their nodes
        if (wave == 0) {
            if (lane == 0) front_publish(lk.nodes + front_node(nbatches, batch, 0), total);
            int64_t acc = total;
            // (front_publishes(batch, j), spelled out: behind the call one constant of this kernel came out in another form)
            for (int j = 1; j < kFrontLevels && ((batch + 1) & (((int64_t)1 << (kFrontFanBits * j)) - 1)) == 0; j++) {
                int64_t x = 0;
                if (lane < kFrontFan - 1) x = front_wait(lk.nodes + front_sibling(nbatches, batch, j, lane));
                acc += wave_reduce(x, R_SUM);              // (lane 0 holds the sums)
                if (lane == 0) front_publish(lk.nodes + front_node(nbatches, batch, j), acc);
            }
        }
        // where the survivors go: one node per unit of each hex digit of the batch number, a lane each
        if (wave == NW - 1) {
            int64_t x = 0;
#define VDL_FRONT_WAIT_AT(word) front_wait(lk.nodes + (word))
            VDL_FRONT_PREFIX_WALK(x, nbatches, batch, lane, VDL_FRONT_WAIT_AT);          // (vdl_front_index.h: the text a host program runs too)
#undef VDL_FRONT_WAIT_AT
            x = wave_reduce(x, R_SUM);
            if (lane == 0) s_off = x;
        }
        __syncthreads();                                   // (also: every tile's positions and carried values are in LDS)
        const int64_t off = s_off;
        if (batch == nbatches - 1 && tid == 0) {
            *lk.total = off + total;
            if (lk.total_host) __hip_atomic_store(lk.total_host, (int64_t)(off + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);    // (the host polls it)
        }
        // the survivors' rows: what the outputs need of them -- fact columns at the row (carried values from LDS), dimension columns
        // through the index -- and the packed vectors.  (Nothing is written beyond the vectors' capacity: the host may have guessed it.)
        // Columns read from images are decoded as they are loaded: everything the take side computes is in the columns' own values.
        if (off < Dtr.out_cap) {
            for (int k = tid; k < total; k += BS) {
                const int64_t row = batch * (kFrontBatch * TILE) + (int64_t)spos[k];
                int64_t vt[NCT][1];
#pragma unroll
                for (int c = 0; c < NCT; c++) {
                    vt[c][0] = 0;
                    if (c < Ct.ncol && ((Dt.take >> c) & 1u) && !((Ct.derived >> c) & 1u)) {
                        if (((Dt.carry >> c) & 1u) && k < kFrontCarry) vt[c][0] = cst[__builtin_popcount(Dt.carry & ((1u << c) - 1u))][k];
                        else if ((Ct.steps >> c) & 1u) vt[c][0] = step_load(Ctr.ptr[c], Ctr.n, Dt.ibase[c], Ct.width(c), row);      // a step image at a random row: two loads
                        else {
                            vt[c][0] = load_scalar(Ctr.ptr[c], Ct.width(c), row);
                            if ((Ct.decode >> c) & 1u) vt[c][0] = img_decode(vt[c][0], Dt.ibase[c], Dt.iscale[c]);
                        }
                    }
                }
                bool on[1] = {true};
                int64_t rid1[1] = {Ctr.row0 + row};
                derive<NCT, 1>(Ct, Ctr, Dt, Dtr, vt, on, Ct.derived & Dt.take, rid1, false);
                if (off + k >= Dtr.out_cap) continue;
                Dtr.out_idx[off + k] = row;
                VDL_SPEC_UNROLL
                for (int o = 0; o < Dt.nout; o++) {
                    const int oc = Dt.out_col[o];
                    int64_t x = 0;
                    if (oc >= 0) {
#pragma unroll
                        for (int c = 0; c < NCT; c++) if (c == oc) x = vt[c][0];
                    } else {
                        // a row expression over the columns, in the two-accumulator program form of the group keys (ProjPlan::exprs)
                        int64_t acc[1] = {0}, tmp[1] = {0};
                        const int at = Dt.expr_at[-2 - oc], len = Dt.expr_len[-2 - oc];
                        VDL_SPEC_UNROLL
                        for (int s = at; s < at + len; s++) {
                            const KeyStep st = Dt.key[s];               // wave-uniform
                            if (st.kind == KeyStep::LOAD) {
#pragma unroll
                                for (int c = 0; c < NCT; c++) if (c == st.col) { if (st.target) tmp[0] = vt[c][0]; else acc[0] = vt[c][0]; }
                            } else if (st.kind == KeyStep::OPK) {
                                if (st.target) key_rows<1>(st.bin, st.const_left, tmp, st.k);
                                else key_rows<1>(st.bin, st.const_left, acc, st.k);
                            } else {
                                key_combine<1>(st.bin, st.const_left, acc, tmp);
                            }
                        }
                        x = acc[0];
                    }
                    Dtr.out_ptr[o][off + k] = x;
                }
            }
        }
        __syncthreads();                                   // (the next batch reuses the LDS areas)
    }
}

}  // namespace
}  // namespace vdl
