// vdl_image.hip -- the two passes that build a column's frame-of-reference image (the rules: vdl_column_image.h): one reduction
// of min, max and the decimal trailing zeros every value shares with the first, then one pass that writes e = (v - base) / scale
// in the image's width.  Both run when a column is created (ingest), never inside a query.  Also the pass that packs a byte image
// to its bit length, and the one pass that builds a step image (k_image_steps).
#include "vdl_device.h"

namespace vdl {

namespace {

__device__ __forceinline__ int64_t load_w(const void *p, int w, int64_t i) {
    switch (w) {
    case 8: return ((const int64_t *)p)[i];
    case 4: return ((const int32_t *)p)[i];
    case 2: return ((const int16_t *)p)[i];
    default: return ((const int8_t *)p)[i];
    }
}

// ordered keys of int64 values for the unsigned atomics
__device__ __forceinline__ unsigned long long okey(int64_t v) { return (unsigned long long)v ^ 0x8000000000000000ull; }

// out[0] = min, out[1] = max (both as okey), out[2] = min over rows of the decimal trailing zeros of |v - v[0]| (19 when equal)
__global__ __launch_bounds__(256) void k_image_stats(const void *col, int w, int64_t n, unsigned long long *out) {
    const int64_t ref = load_w(col, w, 0);
    unsigned long long mn = ~0ull, mx = 0ull, tz = 19;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t v = load_w(col, w, i);
        const unsigned long long k = okey(v);
        mn = k < mn ? k : mn;
        mx = k > mx ? k : mx;
        if (tz > 0) {
            unsigned long long d = v >= ref ? (unsigned long long)v - (unsigned long long)ref : (unsigned long long)ref - (unsigned long long)v;
            if (d != 0) {
                unsigned long long z = 0;
                while (z < tz && d % 10ull == 0) { d /= 10ull; z++; }
                tz = z;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long a = __shfl_xor(mn, off, 64), b = __shfl_xor(mx, off, 64), z = __shfl_xor(tz, off, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        tz = z < tz ? z : tz;
    }
    if ((threadIdx.x & 63u) == 0) {
        atomicMin(&out[0], mn);
        atomicMax(&out[1], mx);
        atomicMin(&out[2], tz);
    }
}

__global__ void k_image_stats_init(unsigned long long *out) { out[0] = ~0ull; out[1] = 0ull; out[2] = 19ull; }

template <typename T>
__global__ __launch_bounds__(256) void k_image_encode(const void *col, int w, int64_t n, int64_t base, int64_t scale, T *img) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (scale == 1) {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
            img[i] = (T)(int64_t)((uint64_t)load_w(col, w, i) - (uint64_t)base);
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
            img[i] = (T)(int64_t)(((uint64_t)load_w(col, w, i) - (uint64_t)base) / (uint64_t)scale);     // (v >= base: the difference is >= 0)
    }
}

// The bit-packed image (vdl_column_image.h, Packed): one thread per (stripe, lane) gathers its lane's 32 values e - emin from the byte
// image and writes the lane's `bits` dwords; consecutive threads are consecutive lanes, so every dword store of a wave is 256
// contiguous bytes.  Rows past n (the padding of the last stripe) are 0.
template <typename T>
__global__ __launch_bounds__(256) void k_image_pack(const T *img, int64_t n, int64_t emin, int bits, uint32_t *out, int64_t lanes) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t mask = bits == 32 ? 0xffffffffull : (1ull << bits) - 1ull;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < lanes; t += stride) {
        const int64_t s = t / 64, l = t % 64;
        uint32_t *dst = out + s * bits * 64 + l;
        uint64_t acc = 0;                                   // bits not yet written, from bit 0 of dword k
        int have = 0, k = 0;
        for (int j = 0; j < 32; j++) {
            const int64_t i = s * 2048 + (int64_t)j * 64 + l;
            const uint64_t e = i < n ? ((uint64_t)(int64_t)img[i] - (uint64_t)emin) & mask : 0ull;
            acc |= e << have;
            have += bits;
            if (have >= 32) { dst[(int64_t)k * 64] = (uint32_t)acc; k++; acc >>= 32; have -= 32; }
        }
        if (have > 0) dst[(int64_t)k * 64] = (uint32_t)acc;      // (32 * bits is a whole number of dwords: never taken)
    }
}

// The step image (vdl_column_image.h, Steps) in one pass: a wave takes 64 rows, a lane its row and the row before it (its
// neighbour's by a shuffle; lane 0 loads the last row of the group before), and the ballot of "differs from the row before" is the
// group's head word.  The anchor is what lane 0 holds of the row before, less the base.  A step other than 0 or 1 raises out[0];
// out[1] = v[0], the base.  Groups at and past `groups` are the padding: no head bits, the anchor of the last row.  Rows of the last
// group past n read row n - 1 and set no bit.  (heads: `padded` words, the anchors behind them; out[0] zeroed by the caller)
__global__ __launch_bounds__(256) void k_image_steps(const void *col, int w, int64_t n, int64_t groups, int64_t padded, uint64_t *heads, uint32_t *anchor,
                                                     unsigned long long *out) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x / 64);
    const int64_t base = load_w(col, w, 0);
    if (blockIdx.x == 0 && threadIdx.x == 0) out[1] = (unsigned long long)base;
    bool raised = false;                                    // (a wave raises the flag once: a column like l_orderkey, where every group holds
                                                            // a wrong step, had every wave of every group queue at that one word -- 106 ms at SF100)
    for (int64_t g = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; g < padded; g += waves) {
        uint64_t head = 0;
        int64_t before = 0;                                 // lane 0: the row before the group's first
        if (g < groups) {
            const int64_t r = g * 64 + lane;
            const bool in = r < n;
            const int64_t v = load_w(col, w, in ? r : n - 1);
            int64_t prev = __shfl_up(v, 1, 64);
            if (lane == 0) prev = g > 0 ? load_w(col, w, r - 1) : v;
            before = prev;
            const bool same = v == prev, step = v > prev && (uint64_t)v - (uint64_t)prev == 1ull;
            head = __ballot(in && !same);
            if (!raised && __ballot(in && !same && !step) != 0ull) {
                if (lane == 0) atomicOr(&out[0], 1ull);
                raised = true;
            }
        } else if (lane == 0) {
            before = load_w(col, w, n - 1);
        }
        if (lane == 0) {
            heads[g] = head;
            anchor[g] = g > 0 ? (uint32_t)((uint64_t)before - (uint64_t)base) : 0u;
        }
    }
}

}  // namespace

hipError_t launch_image_steps(const void *col, int elem_bytes, int64_t n, int64_t padded_groups, void *image, unsigned long long *out2, hipStream_t s) {
    (void)hipGetLastError();
    const int64_t groups = (n + 63) / 64;
    if (n <= 0 || padded_groups < groups) return hipErrorInvalidValue;
    const int grid = (int)std::min<int64_t>((padded_groups + 3) / 4, 256 * 16);
    k_image_steps<<<grid, 256, 0, s>>>(col, elem_bytes, n, groups, padded_groups, (uint64_t *)image, (uint32_t *)((uint64_t *)image + padded_groups), out2);
    return launch_status();
}

hipError_t launch_image_pack(const void *img, int img_bytes, int64_t n, int64_t emin, int bits, void *out, hipStream_t s) {
    (void)hipGetLastError();
    if (n <= 0) return hipSuccess;
    if (bits < 1 || bits > 32) return hipErrorInvalidValue;
    const int64_t lanes = (n + 2047) / 2048 * 64;
    const int grid = (int)std::min<int64_t>((lanes + 255) / 256, 256 * 16);
    switch (img_bytes) {
    case 1: k_image_pack<int8_t><<<grid, 256, 0, s>>>((const int8_t *)img, n, emin, bits, (uint32_t *)out, lanes); break;
    case 2: k_image_pack<int16_t><<<grid, 256, 0, s>>>((const int16_t *)img, n, emin, bits, (uint32_t *)out, lanes); break;
    case 4: k_image_pack<int32_t><<<grid, 256, 0, s>>>((const int32_t *)img, n, emin, bits, (uint32_t *)out, lanes); break;
    case 8: k_image_pack<int64_t><<<grid, 256, 0, s>>>((const int64_t *)img, n, emin, bits, (uint32_t *)out, lanes); break;
    default: return hipErrorInvalidValue;
    }
    return launch_status();
}

hipError_t launch_image_stats(const void *col, int elem_bytes, int64_t n, unsigned long long *out3, hipStream_t s) {
    (void)hipGetLastError();
    if (n <= 0) return hipErrorInvalidValue;
    k_image_stats_init<<<1, 1, 0, s>>>(out3);
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 256 * 8);
    k_image_stats<<<grid, 256, 0, s>>>(col, elem_bytes, n, out3);
    return launch_status();
}

hipError_t launch_image_encode(const void *col, int elem_bytes, int64_t n, int64_t base, int64_t scale, void *img, int img_bytes, hipStream_t s) {
    (void)hipGetLastError();
    if (n <= 0) return hipSuccess;
    if (scale < 1) return hipErrorInvalidValue;
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 256 * 16);
    switch (img_bytes) {
    case 1: k_image_encode<int8_t><<<grid, 256, 0, s>>>(col, elem_bytes, n, base, scale, (int8_t *)img); break;
    case 2: k_image_encode<int16_t><<<grid, 256, 0, s>>>(col, elem_bytes, n, base, scale, (int16_t *)img); break;
    case 4: k_image_encode<int32_t><<<grid, 256, 0, s>>>(col, elem_bytes, n, base, scale, (int32_t *)img); break;
    default: return hipErrorInvalidValue;
    }
    return launch_status();
}

}  // namespace vdl
