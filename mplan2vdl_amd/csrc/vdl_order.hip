// vdl_order.hip -- ORDER BY / LIMIT over the result columns where they lie: in HBM (vdl_plan_set_order).
//
// The order wanted -- keys compared as signed int64, each ascending or descending, ties by the row's position -- is the
// unsigned ascending order of the composite (u_1, .., u_K, position) with u = key ^ flip: flip = 2^63 turns the signed order
// into the unsigned one, flip = 2^63 - 1 does that and complements (descending).  No negation anywhere: INT64_MIN has none.
//
// Top-N (0 < L <= kOrdTopMax): an MSB-first radix select.  Per key reached: one min / max pass over the rows that still match
// (shared leading bits and constant keys cost no round), then rounds of {histogram of the next digit over the matching rows,
// one-block pick of the bin that holds the L'-th row}.  The host drives the rounds (three words back per round through the
// pinned words) and stops as soon as the boundary bin holds at most kOrdBoundary rows; `close` turns what was chosen for a
// key into the two bitmaps {rows strictly below, rows still matching}.  The candidates' positions come out of the existing
// compaction kernels in position order, at most L + kOrdBoundary of them are ranked by counting under the full comparator.
// Full order (L = 0 or L > kOrdTopMax): the engine sorts key by key, last key first, through the one-sweep Partition
// (vdl_partition.hip); what is here for it is the key transform u - min(u) read through the permutation so far, and the
// composition of permutations.  Both end in ONE gather launch that writes every output's rows through the index list.
#include <hip/hip_runtime.h>

#include "vdl_device.h"

namespace vdl {

constexpr int kOrdBlock = 256;
constexpr int kOrdLoads = 4;                   // per lane and loop turn: four independent 16-byte loads in flight, two rows each
constexpr int kOrdRows = 2 * kOrdLoads;
constexpr int kOrdTile = kOrdBlock * kOrdRows;

// the tile's rows of this lane: u[2q], u[2q + 1] = rows base + 2 * (q * kOrdBlock + lane) and the next one (an even row number: one
// aligned 16-byte load, and both rows' bits in one word of `active`)
__device__ __forceinline__ void ord_load_tile(const int64_t *__restrict__ key, uint64_t flip, const uint64_t *__restrict__ active, int64_t m, int64_t base,
                                              uint64_t (&u)[kOrdRows], bool (&ok)[kOrdRows]) {
#pragma unroll
    for (int q = 0; q < kOrdLoads; q++) {
        const int64_t i = base + 2 * ((int64_t)q * kOrdBlock + threadIdx.x);
        ll2 v = {0, 0};
        if (i + 1 < m) v = *(const ll2 *)(key + i);
        else if (i < m) v.x = key[i];
        ok[2 * q] = i < m; ok[2 * q + 1] = i + 1 < m;
        u[2 * q] = (uint64_t)v.x ^ flip; u[2 * q + 1] = (uint64_t)v.y ^ flip;
        if (active) {
            const uint64_t w = i < m ? active[i >> 6] >> (i & 63) : 0;
            ok[2 * q] = ok[2 * q] && (w & 1ull); ok[2 * q + 1] = ok[2 * q + 1] && (w & 2ull);
        }
    }
}

// Grids are capped low: what a block adds at its end goes to addresses every block shares (two words for min / max, the bins that
// occur for a histogram), and same-address atomics from 2048 blocks cost more than the rows' bytes did (order_q3.txt).
static int ord_grid(int64_t m, int cap) { return (int)std::max<int64_t>(1, std::min<int64_t>((m + kOrdTile - 1) / kOrdTile, cap)); }

__device__ __forceinline__ bool ord_match(uint64_t u, int hi_shift, uint64_t prefix) { return hi_shift >= 64 || (u >> hi_shift) == prefix; }

// st[0] = max(~u), st[1] = max(u) over the rows of `active` (null = all): both start at zero, so one memset arms them
__global__ __launch_bounds__(kOrdBlock) void k_ord_minmax(const int64_t *__restrict__ key, uint64_t flip, const uint64_t *__restrict__ active, int64_t m,
                                                          unsigned long long *st) {
    __shared__ uint64_t red[2][kOrdBlock / kWave];
    uint64_t nmin = 0, mx = 0;
    for (int64_t base = (int64_t)blockIdx.x * kOrdTile; base < m; base += (int64_t)gridDim.x * kOrdTile) {
        uint64_t u[kOrdRows];
        bool ok[kOrdRows];
        ord_load_tile(key, flip, active, m, base, u, ok);
#pragma unroll
        for (int r = 0; r < kOrdRows; r++)
            if (ok[r]) { nmin = max(nmin, ~u[r]); mx = max(mx, u[r]); }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        nmin = max(nmin, (uint64_t)__shfl_xor((unsigned long long)nmin, off, kWave));
        mx = max(mx, (uint64_t)__shfl_xor((unsigned long long)mx, off, kWave));
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) { red[0][wave] = nmin; red[1][wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kOrdBlock / kWave; w++) { nmin = max(nmin, red[0][w]); mx = max(mx, red[1][w]); }
        atomicMax(st + 0, (unsigned long long)nmin);
        atomicMax(st + 1, (unsigned long long)mx);
    }
}

// Histogram of digit (u >> shift) & mask over the rows of `active` whose bits from hi_shift up equal `prefix`.  Counts pile up in
// LDS; a wave first folds the lanes that share its first matching lane's digit into ONE add (two ballots), so a digit that
// most rows share costs one LDS atomic per wave instead of 64 on one address.  Then one global add per non-empty bin and block.
__global__ __launch_bounds__(kOrdBlock) void k_ord_hist(const int64_t *__restrict__ key, uint64_t flip, const uint64_t *__restrict__ active, int64_t m,
                                                        int hi_shift, uint64_t prefix, int shift, uint32_t mask, unsigned long long *hist) {
    __shared__ uint32_t h[kOrdBins];
    for (int b = threadIdx.x; b < kOrdBins; b += kOrdBlock) h[b] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    for (int64_t base = (int64_t)blockIdx.x * kOrdTile; base < m; base += (int64_t)gridDim.x * kOrdTile) {
        uint64_t u[kOrdRows];
        bool ok[kOrdRows];
        ord_load_tile(key, flip, active, m, base, u, ok);
#pragma unroll
        for (int r = 0; r < kOrdRows; r++) {
            const bool in = ok[r] && ord_match(u[r], hi_shift, prefix);
            const uint32_t d = (uint32_t)(u[r] >> shift) & mask;
            const uint64_t bal = __ballot(in);
            if (bal == 0) continue;                                        // wave-uniform
            const int leader = __ffsll((unsigned long long)bal) - 1;
            const uint32_t d0 = (uint32_t)__shfl((int)d, leader, kWave);
            const uint64_t same = __ballot(in && d == d0);
            if (in) {
                if (d == d0) { if (lane == leader) atomicAdd(&h[d0], (uint32_t)__popcll((unsigned long long)same)); }
                else atomicAdd(&h[d], 1u);
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kOrdBins; b += kOrdBlock)
        if (h[b]) atomicAdd(hist + b, (unsigned long long)h[b]);
}

// One block: the bin that holds the need-th matching row (1-based, bins ascending) -> st[2] = bin, st[3] = rows in the bins below
// it, st[4] = rows in it; the histogram is left at zero for the next round.
__global__ __launch_bounds__(kOrdBlock) void k_ord_pick(unsigned long long *st, int64_t need) {
    constexpr int PER = kOrdBins / kOrdBlock;
    __shared__ uint64_t sums[kOrdBlock];
    unsigned long long *hist = st + kOrdStateHead;
    uint64_t v[PER], mine = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) { v[k] = hist[threadIdx.x * PER + k]; hist[threadIdx.x * PER + k] = 0; mine += v[k]; }
    sums[threadIdx.x] = mine;
    __syncthreads();
    uint64_t before = 0;
    for (int t = 0; t < (int)threadIdx.x; t++) before += sums[t];          // 256 words out of LDS, broadcast reads
    if (before < (uint64_t)need && (uint64_t)need <= before + mine) {      // exactly one thread, when need <= the rows counted
#pragma unroll
        for (int k = 0; k < PER; k++) {
            if (before < (uint64_t)need && (uint64_t)need <= before + v[k]) { st[2] = threadIdx.x * PER + k; st[3] = before; st[4] = v[k]; }
            before += v[k];
        }
    }
}

// What the rounds chose for one key, as bitmaps: a row of `active_in` (null = all) whose bits from hi_shift up are below / equal to
// `prefix` goes into `below` (OR-ed in: it holds the rows earlier keys put there) / `active_out`.  One wave per 64 rows: the
// ballot IS the bitmap word, and the key is read coalesced.
__global__ __launch_bounds__(kOrdBlock) void k_ord_close(const int64_t *__restrict__ key, uint64_t flip, const uint64_t *__restrict__ active_in, int64_t m,
                                                         int hi_shift, uint64_t prefix, uint64_t *__restrict__ active_out, uint64_t *__restrict__ below) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t nw = (m + 63) >> 6;
    const int64_t wave0 = ((int64_t)blockIdx.x * kOrdBlock + threadIdx.x) / kWave, nwaves = (int64_t)gridDim.x * (kOrdBlock / kWave);
    for (int64_t w = wave0; w < nw; w += nwaves) {
        const int64_t i = (w << 6) + lane;
        bool in = i < m;
        const uint64_t u = in ? (uint64_t)key[i] ^ flip : 0;
        const uint64_t aw = active_in ? active_in[w] : ~0ull;
        in = in && ((aw >> lane) & 1ull);
        const uint64_t top = u >> hi_shift;                                // hi_shift < 64: a key is closed after at least one round
        const uint64_t eq = __ballot(in && top == prefix), lt = __ballot(in && top < prefix);
        if (lane == 0) { active_out[w] = eq; below[w] |= lt; }
    }
}

// the candidates' keys, transformed, key-major: ck[k * n + i] = u_k(row pos[i])
__global__ __launch_bounds__(kOrdBlock) void k_ord_stage(OrdKeys K, const int64_t *__restrict__ pos, int64_t n, uint64_t *__restrict__ ck) {
    const int64_t i = (int64_t)blockIdx.x * kOrdBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t row = pos[i];
    for (int k = 0; k < K.n; k++) ck[(int64_t)k * n + i] = (uint64_t)K.key[k][row] ^ K.flip[k];
}

// rank of every candidate = how many candidates come before it under (u_1, .., u_K, position); the first `keep` ranks are the answer
__global__ __launch_bounds__(kOrdBlock) void k_ord_rank(const uint64_t *__restrict__ ck, const int64_t *__restrict__ pos, int nk, int64_t n, int64_t keep,
                                                        int64_t *__restrict__ index_out) {
    __shared__ uint64_t tk[kOrdMaxKeys][kOrdBlock];
    __shared__ int64_t tp[kOrdBlock];
    const int64_t i = (int64_t)blockIdx.x * kOrdBlock + threadIdx.x;
    const bool have = i < n;
    uint64_t mine[kOrdMaxKeys];
#pragma unroll
    for (int k = 0; k < kOrdMaxKeys; k++) mine[k] = (have && k < nk) ? ck[(int64_t)k * n + i] : 0;
    const int64_t mypos = have ? pos[i] : 0;
    int64_t rank = 0;
    for (int64_t t0 = 0; t0 < n; t0 += kOrdBlock) {
        const int64_t j = t0 + threadIdx.x;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kOrdMaxKeys; k++)
            if (k < nk) tk[k][threadIdx.x] = j < n ? ck[(int64_t)k * n + j] : 0;
        tp[threadIdx.x] = j < n ? pos[j] : 0;
        __syncthreads();
        const int cnt = (int)min((int64_t)kOrdBlock, n - t0);
        for (int q = 0; q < cnt; q++) {
            bool less = false, decided = false;
#pragma unroll
            for (int k = 0; k < kOrdMaxKeys; k++) {
                if (k < nk) {
                    const uint64_t o = tk[k][q];                           // the same address in every lane: a broadcast
                    less = decided ? less : o < mine[k];
                    decided = decided || o != mine[k];
                }
            }
            if (!decided) less = tp[q] < mypos;
            rank += less ? 1 : 0;
        }
    }
    if (have && rank < keep) index_out[rank] = mypos;
}

// every output's rows through the index list, one launch: blockIdx.y = output
__global__ __launch_bounds__(kOrdBlock) void k_ord_gather(OrdGather G, const int64_t *__restrict__ index, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kOrdBlock + threadIdx.x;
    if (i >= n) return;
    G.dst[blockIdx.y][i] = G.src[blockIdx.y][index[i]];
}

// ---- sharded runs: the candidate block a rank contributes, and the merge of the gathered blocks ----
// blockIdx.y = column of the block: an order word or an output, the chosen rows in the rank's sorted order
__global__ __launch_bounds__(kOrdBlock) void k_ord_block(OrdBlock B, const int64_t *__restrict__ index, int64_t n, int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kOrdBlock + threadIdx.x;
    if (i >= n) return;
    const int c = blockIdx.y;
    out[(int64_t)c * n + i] = (int64_t)((uint64_t)B.src[c][index ? index[i] : i] ^ B.flip[c]);
}

// The merge (ord_merge_place, vdl_kernels.h): one lane per gathered candidate, no atomics, nothing comes back to the host.  At most
// world * kOrdTopMax candidates: a latency-bound kernel of some hundred waves whose searches read K columns of at most a few MB --
// L2-resident after the first touch.  One wave per block spreads those waves over the CUs (128 blocks of 256 would leave half the chip
// idle at eight ranks).  The runs' first words are NOT staged in LDS: eight runs of 4096 words are 256 KiB, more than a CU's 160 KiB,
// and a sampled top of each search tree would save two or three of twelve dependent L2 reads per run for one more barrier and a
// fill that every block repeats.
constexpr int kOrdMergeBlock = 64;
__global__ __launch_bounds__(kOrdMergeBlock) void k_ord_merge(OrdRuns R, OrdGather G, const uint64_t *__restrict__ w, int64_t keep) {
    const int64_t N = R.off[R.world];
    const int64_t j = (int64_t)blockIdx.x * kOrdMergeBlock + threadIdx.x;
    if (j >= N) return;
    const int64_t place = ord_merge_place(R, w, j);
    if (place >= keep) return;
    for (int o = 0; o < G.n; o++) G.dst[o][place] = G.src[o][j];
}

// full order: the sort key of the row that stands at place i so far -- u - umin whole (half 0), its low (1) or high (2) 32 bits
__global__ __launch_bounds__(kOrdBlock) void k_ord_sortkey(const int64_t *__restrict__ key, uint64_t flip, const int64_t *__restrict__ perm, int64_t m,
                                                           uint64_t umin, int half, int64_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kOrdBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kOrdBlock) {
        const uint64_t t = ((uint64_t)key[perm ? perm[i] : i] ^ flip) - umin;
        out[i] = (int64_t)(half == 0 ? t : half == 1 ? (t & 0xffffffffull) : (t >> 32));
    }
}
__global__ __launch_bounds__(kOrdBlock) void k_ord_compose(const int64_t *__restrict__ perm, const int64_t *__restrict__ order, int64_t m, int64_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kOrdBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kOrdBlock) out[i] = perm[order[i]];
}

hipError_t launch_order_minmax(const int64_t *key, uint64_t flip, const uint64_t *active, int64_t m, uint64_t *state, hipStream_t s) {
    (void)hipGetLastError();
    if (m <= 0) return hipSuccess;
    k_ord_minmax<<<ord_grid(m, 512), kOrdBlock, 0, s>>>(key, flip, active, m, (unsigned long long *)state);
    return launch_status();
}
hipError_t launch_order_round(const int64_t *key, uint64_t flip, const uint64_t *active, int64_t m, int hi_shift, uint64_t prefix, int shift, int width,
                              int64_t need, uint64_t *state, hipStream_t s) {
    (void)hipGetLastError();
    if (m <= 0 || width < 1 || width > kOrdDigitBits || shift < 0 || shift + width > 64 || need < 1) return hipErrorInvalidValue;
    k_ord_hist<<<ord_grid(m, 1024), kOrdBlock, 0, s>>>(key, flip, active, m, hi_shift, prefix, shift, (1u << width) - 1u, (unsigned long long *)state + kOrdStateHead);
    k_ord_pick<<<1, kOrdBlock, 0, s>>>((unsigned long long *)state, need);
    return launch_status();
}
hipError_t launch_order_close(const int64_t *key, uint64_t flip, const uint64_t *active_in, int64_t m, int hi_shift, uint64_t prefix, uint64_t *active_out,
                              uint64_t *below, hipStream_t s) {
    (void)hipGetLastError();
    if (m <= 0) return hipSuccess;
    if (hi_shift < 0 || hi_shift > 63) return hipErrorInvalidValue;
    const int64_t nw = (m + 63) >> 6;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((nw + 3) / 4, 4096));
    k_ord_close<<<grid, kOrdBlock, 0, s>>>(key, flip, active_in, m, hi_shift, prefix, active_out, below);
    return launch_status();
}
hipError_t launch_order_rank(const OrdKeys &K, const int64_t *pos, int64_t n, int64_t keep, uint64_t *staged, int64_t *index_out, hipStream_t s) {
    (void)hipGetLastError();
    if (n <= 0) return hipSuccess;
    if (K.n < 0 || K.n > kOrdMaxKeys || n > kOrdTopMax + kOrdBoundary) return hipErrorInvalidValue;
    const int grid = (int)((n + kOrdBlock - 1) / kOrdBlock);
    if (K.n > 0) k_ord_stage<<<grid, kOrdBlock, 0, s>>>(K, pos, n, staged);
    k_ord_rank<<<grid, kOrdBlock, 0, s>>>(staged, pos, K.n, n, keep, index_out);
    return launch_status();
}
hipError_t launch_order_gather(const OrdGather &G, const int64_t *index, int64_t n, hipStream_t s) {
    (void)hipGetLastError();
    if (n <= 0 || G.n <= 0) return hipSuccess;
    if (G.n > kOrdGatherMax) return hipErrorInvalidValue;
    k_ord_gather<<<dim3((unsigned)((n + kOrdBlock - 1) / kOrdBlock), (unsigned)G.n), kOrdBlock, 0, s>>>(G, index, n);
    return launch_status();
}
hipError_t launch_order_block(const OrdBlock &B, const int64_t *index, int64_t n, int64_t *out, hipStream_t s) {
    (void)hipGetLastError();
    if (n <= 0 || B.n <= 0) return hipSuccess;
    if (B.n > kOrdBlockCols || !out) return hipErrorInvalidValue;
    k_ord_block<<<dim3((unsigned)((n + kOrdBlock - 1) / kOrdBlock), (unsigned)B.n), kOrdBlock, 0, s>>>(B, index, n, out);
    return launch_status();
}
hipError_t launch_order_merge(const OrdRuns &R, const OrdGather &G, const uint64_t *w, int64_t keep, hipStream_t s) {
    (void)hipGetLastError();
    if (R.world < 1 || R.world > kMaxExWorld || R.nk < 0 || R.nk > kOrdMaxKeys || G.n < 0 || G.n > kOrdGatherMax || R.off[0] != 0) return hipErrorInvalidValue;
    for (int r = 0; r < R.world; r++) if (R.off[r + 1] < R.off[r]) return hipErrorInvalidValue;
    const int64_t N = R.off[R.world];
    if (N <= 0 || keep <= 0 || G.n == 0) return hipSuccess;
    if (!w && R.nk > 0) return hipErrorInvalidValue;
    k_ord_merge<<<(unsigned)((N + kOrdMergeBlock - 1) / kOrdMergeBlock), kOrdMergeBlock, 0, s>>>(R, G, w, keep);
    return launch_status();
}
hipError_t launch_order_sortkey(const int64_t *key, uint64_t flip, const int64_t *perm, int64_t m, uint64_t umin, int half, int64_t *out, hipStream_t s) {
    (void)hipGetLastError();
    if (m <= 0) return hipSuccess;
    k_ord_sortkey<<<(int)std::min<int64_t>((m + kOrdBlock - 1) / kOrdBlock, 4096), kOrdBlock, 0, s>>>(key, flip, perm, m, umin, half, out);
    return launch_status();
}
hipError_t launch_order_compose(const int64_t *perm, const int64_t *order, int64_t m, int64_t *out, hipStream_t s) {
    (void)hipGetLastError();
    if (m <= 0) return hipSuccess;
    k_ord_compose<<<(int)std::min<int64_t>((m + kOrdBlock - 1) / kOrdBlock, 4096), kOrdBlock, 0, s>>>(perm, order, m, out);
    return launch_status();
}

}  // namespace vdl
