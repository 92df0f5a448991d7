// vdl_collate.hip -- the collation index of a string heap: heap offset -> dense rank of the string in text order.
//
// A heap is one byte per slot, NUL-terminated strings wherever dictionary.csv put them.  Text order is strcmp on UNSIGNED bytes.  The
// index is built once per heap column in five steps, each a kernel here, driven by collation_build (vdl_collate.cpp):
//   mark    one lane per byte: bit i of the start bitmap = heap[i] != 0 and (i == 0 or heap[i - 1] == 0); the ballot is the bitmap word.
//           The starts are compacted to an offset list by the engine's own popcount / compact_write.
//   lengths one lane per string: the longest string, and the OR of all start offsets (its low bits give the table's granularity)
//   words   one lane per string: word j = bytes [8j, 8j + 8) big-endian, zero from the NUL on, so that the unsigned order of
//           (word 0, word 1, ..) IS the text order.  Aligned 8-byte loads, two neighbours funnelled together for an unaligned start.
//   sort    least significant word first through the stable Partition path of the order step (no kernel of its own)
//   heads   flag r = the string at sorted place r differs from its predecessor; an exclusive scan of the flags gives the ranks
//   table   slot s of the table stands for heap offset s << gshift: 0 where that byte is NUL, the rank where a string starts, -1 else
// and k_ord_textkey translates a key column of codes into ranks for the order step: one isolated table fetch per row.
#include <hip/hip_runtime.h>

#include "vdl_device.h"

namespace vdl {

constexpr int kColBlock = 256;

__device__ __forceinline__ uint64_t wave_or(uint64_t x) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) x |= (uint64_t)__shfl_xor((unsigned long long)x, off, kWave);
    return x;
}
__device__ __forceinline__ int64_t wave_max(int64_t x) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) x = max(x, (int64_t)__shfl_xor((long long)x, off, kWave));
    return x;
}
__device__ __forceinline__ int64_t wave_min(int64_t x) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) x = min(x, (int64_t)__shfl_xor((long long)x, off, kWave));
    return x;
}

// One wave per 64 bytes.  The byte before a lane's own is its left neighbour's; lane 0 reads the one before the wave's first from
// memory (another wave's or block's byte: read, never assumed).
__global__ __launch_bounds__(kColBlock) void k_col_mark(const int8_t *__restrict__ heap, int64_t n, uint64_t *__restrict__ starts) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t nw = (n + 63) >> 6;
    const int64_t wave0 = ((int64_t)blockIdx.x * kColBlock + threadIdx.x) / kWave, nwaves = (int64_t)gridDim.x * (kColBlock / kWave);
    for (int64_t w = wave0; w < nw; w += nwaves) {
        const int64_t i = (w << 6) + lane;
        const int b = i < n ? heap[i] : 0;
        int prev = __shfl_up(b, 1, kWave);
        if (lane == 0) prev = i > 0 ? heap[i - 1] : 0;
        const uint64_t bal = __ballot(i < n && b != 0 && prev == 0);
        if (lane == 0) starts[w] = bal;
    }
}

// st[0] = longest string in bytes, st[1] = OR of the start offsets (both zero before).  The NUL that ends string i lies before the
// next start (a start's predecessor is NUL) or the heap ends first: the walk stays inside [off[i], end).
__global__ __launch_bounds__(kColBlock) void k_col_lengths(const int8_t *__restrict__ heap, int64_t n, const int64_t *__restrict__ off, int64_t d,
                                                           unsigned long long *st) {
    int64_t longest = 0;
    uint64_t bits = 0;
    for (int64_t i = (int64_t)blockIdx.x * kColBlock + threadIdx.x; i < d; i += (int64_t)gridDim.x * kColBlock) {
        const int64_t s = off[i], end = i + 1 < d ? off[i + 1] : n;
        int64_t e = s;
        while (e < end && heap[e] != 0) e++;
        longest = max(longest, e - s);
        bits |= (uint64_t)s;
    }
    longest = wave_max(longest);
    bits = wave_or(bits);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (longest) atomicMax(st + 0, (unsigned long long)longest);
        if (bits) atomicOr(st + 1, (unsigned long long)bits);
    }
}

// the eight bytes at heap offsets [a, a + 8), byte a lowest; heap + a is 8-byte aligned.  Offsets outside [0, n) read as NUL: nothing
// outside the heap is touched (the word that holds the heap's first or last bytes is put together byte by byte)
__device__ __forceinline__ uint64_t col_load8(const int8_t *__restrict__ heap, int64_t n, int64_t a) {
    if (a >= 0 && a + 8 <= n) return *(const uint64_t *)(heap + a);
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int64_t q = a + k;
        if (q >= 0 && q < n) v |= (uint64_t)(uint8_t)heap[q] << (8 * k);
    }
    return v;
}

// words[j * d + i] = word j of string i, j < nwords (nwords * 8 >= the longest string)
__global__ __launch_bounds__(kColBlock) void k_col_words(const int8_t *__restrict__ heap, int64_t n, const int64_t *__restrict__ off, int64_t d, int nwords,
                                                         uint64_t *__restrict__ words) {
    for (int64_t i = (int64_t)blockIdx.x * kColBlock + threadIdx.x; i < d; i += (int64_t)gridDim.x * kColBlock) {
        const int64_t s = off[i];
        const int mis = (int)(((uintptr_t)heap + (uintptr_t)s) & 7), sh = 8 * mis;
        const int64_t a0 = s - mis;
        uint64_t cur = col_load8(heap, n, a0);
        bool done = false;
        for (int j = 0; j < nwords; j++) {
            uint64_t v = 0;
            if (!done) {
                const uint64_t nxt = col_load8(heap, n, a0 + 8 * (int64_t)(j + 1));
                v = mis ? (cur >> sh) | (nxt << (64 - sh)) : cur;
                cur = nxt;
                // the lowest flagged byte of the classic zero-byte test is exactly the first NUL: everything from it on belongs to
                // the padding or to the next string
                const uint64_t t = (v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull;
                if (t) {
                    const int at = (__ffsll((unsigned long long)t) - 1) >> 3;
                    v = at ? v & (~0ull >> (64 - 8 * at)) : 0;
                    done = true;
                }
            }
            words[(int64_t)j * d + i] = __builtin_bswap64(v);
        }
    }
}

// flags[r] = 1 when the string at sorted place r starts a new run of equal strings (r = 0 does), flags[d] = 0: after an exclusive
// scan over the d + 1 entries flags[r + 1] is the dense rank (from 1) of place r, and flags[d] the number of distinct strings
__global__ __launch_bounds__(kColBlock) void k_col_heads(const uint64_t *__restrict__ words, const int64_t *__restrict__ perm, int64_t d, int nwords,
                                                         int64_t *__restrict__ flags) {
    for (int64_t r = (int64_t)blockIdx.x * kColBlock + threadIdx.x; r < d; r += (int64_t)gridDim.x * kColBlock) {
        bool head = r == 0;
        if (!head) {
            const int64_t a = perm ? perm[r] : r, b = perm ? perm[r - 1] : r - 1;
            for (int j = 0; j < nwords && !head; j++) head = words[(int64_t)j * d + a] != words[(int64_t)j * d + b];
        }
        flags[r] = head ? 1 : 0;
        if (r == d - 1) flags[d] = 0;
    }
}

// every slot of the table: 0 where the byte it stands for is NUL (the empty string), -1 (not a start) otherwise
__global__ __launch_bounds__(kColBlock) void k_col_table_init(const int8_t *__restrict__ heap, int64_t n, int gshift, int64_t slots, int32_t *__restrict__ table) {
    for (int64_t t = (int64_t)blockIdx.x * kColBlock + threadIdx.x; t < slots; t += (int64_t)gridDim.x * kColBlock)
        table[t] = heap[t << gshift] == 0 ? 0 : -1;
}
// ... and the rank of the string at sorted place r at its start's slot (ranks = the scanned flags: rank of place r at ranks[r + 1])
__global__ __launch_bounds__(kColBlock) void k_col_table_ranks(const int64_t *__restrict__ off, const int64_t *__restrict__ perm, const int64_t *__restrict__ ranks,
                                                               int64_t d, int gshift, int32_t *__restrict__ table) {
    for (int64_t r = (int64_t)blockIdx.x * kColBlock + threadIdx.x; r < d; r += (int64_t)gridDim.x * kColBlock)
        table[off[perm ? perm[r] : r] >> gshift] = (int32_t)ranks[r + 1];
}

// The order step's text key: ranks[i] = rank of the string code[i] names.  A code on the table's grid is answered by the table alone
// (one isolated 4-byte fetch); a code between its slots can only be a NUL byte (rank 0) or the middle of a string.  Codes that are no
// string of this heap -- negative, at or past the end, mid-string -- get -1, are counted in st[0], and st[1] = max(~row) over them:
// the complement of the first such row (both words zero before, so one memset arms them).
__global__ __launch_bounds__(kColBlock) void k_ord_textkey(const int64_t *__restrict__ code, int64_t m, const int8_t *__restrict__ heap, int64_t n,
                                                           const int32_t *__restrict__ table, int gshift, int64_t *__restrict__ ranks, unsigned long long *st) {
    int64_t bad = 0, first = INT64_MAX;
    const int64_t gmask = ((int64_t)1 << gshift) - 1;
    for (int64_t i = (int64_t)blockIdx.x * kColBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kColBlock) {
        const int64_t c = code[i];
        int64_t r = -1;
        if (c >= 0 && c < n) {
            if ((c & gmask) == 0) r = table[c >> gshift];
            else if (heap[c] == 0) r = 0;
        }
        ranks[i] = r;
        if (r < 0) { bad++; first = min(first, i); }
    }
    const bool any = __ballot(bad != 0) != 0;                         // wave-uniform: the usual run has no such row and adds nothing
    if (any) {
        bad = wave_reduce(bad, R_SUM);
        first = wave_min(first);
        if ((threadIdx.x & (kWave - 1)) == 0) {
            atomicAdd(st + 0, (unsigned long long)bad);
            atomicMax(st + 1, ~(unsigned long long)first);
        }
    }
}

static int col_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + kColBlock - 1) / kColBlock, 4096)); }

hipError_t launch_collate_mark(const int8_t *heap, int64_t n, uint64_t *starts, hipStream_t s) {
    (void)hipGetLastError();
    if (n <= 0) return hipSuccess;
    const int64_t nw = (n + 63) >> 6;
    k_col_mark<<<(int)std::max<int64_t>(1, std::min<int64_t>((nw + 3) / 4, 4096)), kColBlock, 0, s>>>(heap, n, starts);
    return launch_status();
}
hipError_t launch_collate_lengths(const int8_t *heap, int64_t n, const int64_t *off, int64_t d, uint64_t *state, hipStream_t s) {
    (void)hipGetLastError();
    if (d <= 0) return hipSuccess;
    k_col_lengths<<<col_grid(d), kColBlock, 0, s>>>(heap, n, off, d, (unsigned long long *)state);
    return launch_status();
}
hipError_t launch_collate_words(const int8_t *heap, int64_t n, const int64_t *off, int64_t d, int nwords, uint64_t *words, hipStream_t s) {
    (void)hipGetLastError();
    if (d <= 0) return hipSuccess;
    if (nwords < 1 || nwords > kCollateMaxBytes / 8) return hipErrorInvalidValue;
    k_col_words<<<col_grid(d), kColBlock, 0, s>>>(heap, n, off, d, nwords, words);
    return launch_status();
}
hipError_t launch_collate_heads(const uint64_t *words, const int64_t *perm, int64_t d, int nwords, int64_t *flags, hipStream_t s) {
    (void)hipGetLastError();
    if (d <= 0) return hipSuccess;
    k_col_heads<<<col_grid(d), kColBlock, 0, s>>>(words, perm, d, nwords, flags);
    return launch_status();
}
hipError_t launch_collate_table(const int8_t *heap, int64_t n, int gshift, const int64_t *off, const int64_t *perm, const int64_t *ranks, int64_t d, int32_t *table,
                                hipStream_t s) {
    (void)hipGetLastError();
    if (n <= 0) return hipSuccess;
    if (gshift < 0 || gshift > 3) return hipErrorInvalidValue;
    const int64_t slots = collate_table_slots(n, gshift);
    k_col_table_init<<<col_grid(slots), kColBlock, 0, s>>>(heap, n, gshift, slots, table);
    if (d > 0) k_col_table_ranks<<<col_grid(d), kColBlock, 0, s>>>(off, perm, ranks, d, gshift, table);
    return launch_status();
}
hipError_t launch_order_textkey(const int64_t *code, int64_t m, const int8_t *heap, int64_t n, const int32_t *table, int gshift, int64_t *ranks, uint64_t *state,
                                hipStream_t s) {
    (void)hipGetLastError();
    if (m <= 0) return hipSuccess;
    if (gshift < 0 || gshift > 3) return hipErrorInvalidValue;
    k_ord_textkey<<<(int)std::max<int64_t>(1, std::min<int64_t>((m + kColBlock - 1) / kColBlock, 8192)), kColBlock, 0, s>>>(code, m, heap, n, table, gshift, ranks,
                                                                                                                      (unsigned long long *)state);
    return launch_status();
}

}  // namespace vdl
