// vdl_image.hip -- the two passes that build a column's frame-of-reference image (the rules: vdl_column_image.h): one reduction
// of min, max and the decimal trailing zeros every value shares with the first, then one pass that writes e = (v - base) / scale
// in the image's width.  Both run when a column is created (ingest), never inside a query.
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

}  // namespace

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
