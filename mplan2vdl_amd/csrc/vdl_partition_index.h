// vdl_partition_index.h -- the index arithmetic of the Partition's look-back (vdl_partition.hip): which status row holds which node of
// the fan-out-16 Fenwick tree over the tiles, which rows make up a tile's prefix, and which tile publishes which level.  Pure
// functions of the tile numbers, shared by the kernels and by a host program that plays the protocol through for tile counts no
// device test reaches (tools/sanitize/partition_index_main.cpp, built with ASan + UBSan by tests/test_partition_index_cpu.py).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VDL_PART_INDEX_FN __device__ __forceinline__
#define VDL_PART_INDEX_HOST_FN __host__ __device__ static inline
#else
#define VDL_PART_INDEX_FN static inline
#define VDL_PART_INDEX_HOST_FN static inline
#endif

namespace vdl {

constexpr int kFanBits = 4, kFan = 1 << kFanBits, kFenLevels = 6;            // tiles < 16^6 (launch_partition checks)
// launch_partition refuses a Partition of this many tiles or more.  Tile numbers up to 16^6 - 1 have the six hex digits the prefix is made
// of, so 16^6 tiles would still be served; tile 16^6 is the first whose prefix the rows cannot express (its digits 0 .. 5 are all zero).
constexpr int64_t kFenTileLimit = (int64_t)1 << (kFanBits * kFenLevels);

// row of node (u, level) in a pass's rows: level j holds the tiles u with 16^j | u + 1, in order
VDL_PART_INDEX_HOST_FN int64_t partition_rows(int64_t ntiles) { int64_t r = 0; for (int j = 0; j < kFenLevels; j++) r += ntiles >> (kFanBits * j); return r; }
VDL_PART_INDEX_FN int64_t fen_row(int64_t ntiles, int64_t u, int level) {
    int64_t base = 0;
    for (int j = 0; j < level; j++) base += ntiles >> (kFanBits * j);
    return base + ((u + 1) >> (kFanBits * level)) - 1;
}
// tile u makes the row of level j (the counts of the 16^j tiles ending at u) iff 16^j divides u + 1.  (part_pass_tile spells this
// expression out in its loop over the levels: behind a call the compiler allocated the pass's registers differently.)
VDL_PART_INDEX_FN bool fen_publishes(int64_t u, int level) { return ((u + 1) & (((int64_t)1 << (kFanBits * level)) - 1)) == 0; }
// the i-th row of the prefix of tile t: one row per unit of each hex digit of t
VDL_PART_INDEX_FN int fen_prefix_rows(int64_t t) { int r = 0; for (int j = 0; j < kFenLevels; j++) r += (int)((t >> (kFanBits * j)) & (kFan - 1)); return r; }
VDL_PART_INDEX_FN int64_t fen_prefix_row(int64_t ntiles, int64_t t, int i) {
    for (int j = 0; j < kFenLevels; j++) {
        const int v = (int)((t >> (kFanBits * j)) & (kFan - 1));
        if (i < v) {
            const int64_t hi = t & ~(((int64_t)kFan << (kFanBits * j)) - 1);
            return fen_row(ntiles, hi + ((int64_t)(i + 1) << (kFanBits * j)) - 1, j);
        }
        i -= v;
    }
    return 0;   // not reached
}

}  // namespace vdl
