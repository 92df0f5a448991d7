// partition_index_main.cpp -- the look-back of the radix Partition (vdl_partition.hip: k_part_pass) played through on the host with ONE
// count per tile instead of 256, over the very index functions the kernel uses (vdl_partition_index.h); built with ASan + UBSan by
// tests/test_partition_index_cpu.py.
//
// For a number of tiles:
//   * every tile u stores row (u, 0) = its own count and, for j = 1, 2, ... while 16^j divides u + 1, row (u, j) = row (u, j - 1) plus the 15
//     rows fen_row(u - (i + 1) * 16^(j-1), j - 1) -- the loop of part_pass_tile;
//   * the prefix of tile t is the sum of the rows fen_prefix_row(ntiles, t, i), i < fen_prefix_rows(t), and must equal the plain sum of
//     the counts of the tiles before t;
//   * every row read or written lies in [0, partition_rows(ntiles)); no two nodes share a row; a row that is read has been stored by some
//     tile (the kernel would poll a row nobody stores for ever) and by a tile with a SMALLER number than the reader's (tiles take their
//     numbers from a counter, so those are the tiles known to be running).
// Counts are random 31-bit numbers, so sums reach the 64-bit range of the wide status words.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vdl_partition_index.h"

using namespace vdl;

static long long checks = 0;
static void fail(const char *what, long long ntiles, long long a, long long b, long long c) {
    std::printf("FAIL %s: %lld tiles (%lld, %lld, %lld)\n", what, ntiles, a, b, c);
    std::exit(1);
}
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

struct Rows {
    int64_t ntiles, nrows;
    std::vector<uint64_t> value;
    std::vector<int64_t> owner;          // the tile that stored the row, -1: nobody has
    std::vector<signed char> level;
    explicit Rows(int64_t nt) : ntiles(nt), nrows(partition_rows(nt)), value((size_t)nrows, 0), owner((size_t)nrows, -1), level((size_t)nrows, -1) {}
    void store(int64_t u, int j, uint64_t v) {
        const int64_t r = fen_row(ntiles, u, j);
        if (r < 0 || r >= nrows) fail("a row is stored outside the rows", ntiles, u, j, r);
        if (owner[(size_t)r] >= 0) fail("two nodes share a row", ntiles, u, j, r);
        owner[(size_t)r] = u; level[(size_t)r] = (signed char)j; value[(size_t)r] = v;
        checks += 2;
    }
    uint64_t load(int64_t r, int64_t reader, const char *who) {
        if (r < 0 || r >= nrows) fail(who, ntiles, reader, r, nrows);
        if (owner[(size_t)r] < 0) fail("a row is read that no tile stores (the kernel would wait for ever)", ntiles, reader, r, 0);
        if (owner[(size_t)r] >= reader) fail("a tile waits for a row of a tile that is not before it", ntiles, reader, r, owner[(size_t)r]);
        checks += 3;
        return value[(size_t)r];
    }
};

// `every`: the prefix of every tile is checked (else: the first and last 70 000 and every 251st in between)
static void run(int64_t ntiles, bool every) {
    std::vector<uint64_t> count((size_t)ntiles);
    for (auto &c : count) c = rnd() & 0x7fffffffull;
    Rows R(ntiles);
    // ---- publication, tile by tile in ticket order: a tile reads rows of earlier tiles only, so this order finds them all stored
    for (int64_t u = 0; u < ntiles; u++) {
        uint64_t acc = count[(size_t)u];
        R.store(u, 0, acc);
        if (!fen_publishes(u, 1)) continue;
        for (int j = 1; j < kFenLevels && fen_publishes(u, j); j++) {
            const int64_t step = (int64_t)1 << (kFanBits * (j - 1));
            for (int i = 0; i < kFan - 1; i++) {
                const int64_t sib = u - (int64_t)(i + 1) * step;
                if (sib < 0) fail("a sibling before tile 0", ntiles, u, j, sib);
                const int64_t r = fen_row(ntiles, sib, j - 1);
                if (R.level[(size_t)(r >= 0 && r < R.nrows ? r : 0)] != j - 1) fail("a sibling's row is of another level", ntiles, u, j, r);
                acc += R.load(r, u, "a sibling's row lies outside the rows");
            }
            R.store(u, j, acc);
        }
    }
    // every level-0 row is taken, and the rows are exactly as many as the nodes
    int64_t stored = 0;
    for (int64_t r = 0; r < R.nrows; r++) stored += R.owner[(size_t)r] >= 0;
    int64_t nodes = 0;
    for (int64_t u = 0; u < ntiles; u++) for (int j = 0; j < kFenLevels && fen_publishes(u, j); j++) nodes++;
    if (stored != nodes || stored != R.nrows) fail("rows, nodes and stored rows differ in number", ntiles, R.nrows, nodes, stored);
    // ---- the prefixes
    uint64_t before = 0;
    for (int64_t t = 0; t < ntiles; t++) {
        if (every || t < 70000 || t >= ntiles - 70000 || t % 251 == 0) {
            const int n = fen_prefix_rows(t);
            if (n < 0 || n > kFenLevels * (kFan - 1)) fail("rows of a prefix", ntiles, t, n, 0);
            uint64_t sum = 0;
            for (int i = 0; i < n; i++) sum += R.load(fen_prefix_row(ntiles, t, i), t, "a prefix row lies outside the rows");
            if (sum != before) fail("prefix", ntiles, t, (long long)sum, (long long)before);
            checks++;
        }
        before += count[(size_t)t];
    }
}

int main() {
    static_assert(kFan == 16 && kFenLevels == 6, "the tile counts below are chosen for six levels of fan-out 16");
    for (int64_t ntiles : {(int64_t)1, (int64_t)15, (int64_t)16, (int64_t)17, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)0x111, (int64_t)0xFFF,
                           (int64_t)0x1000, (int64_t)0x1001, (int64_t)0xFFFF, (int64_t)0x10000, (int64_t)0x10001, (int64_t)0xFFFFF, (int64_t)0x100000 + 17})
        run(ntiles, true);
    // ---- the limit.  launch_partition refuses kFenTileLimit tiles and more.  Every tile number below the limit is the sum of its six hex
    // digits' units, which is what the prefix rows express; tile kFenTileLimit is the first whose prefix they cannot (no rows at all, though
    // tiles come before it), so kFenTileLimit + 1 tiles is the first count that would go wrong and the limit is on the safe side of it by one.
    if (kFenTileLimit != (int64_t)1 << (kFanBits * kFenLevels)) fail("the limit", kFenTileLimit, 0, 0, 0);
    for (int64_t t : {kFenTileLimit - 1, kFenTileLimit - 2, kFenTileLimit - kFan, kFenTileLimit >> kFanBits}) {
        int64_t covered = 0;                                  // tiles the prefix rows of t stand for
        int i = 0;
        for (int j = 0; j < kFenLevels; j++) {
            const int v = (int)((t >> (kFanBits * j)) & (kFan - 1));
            covered += (int64_t)v << (kFanBits * j);
            i += v;
        }
        if (covered != t || i != fen_prefix_rows(t)) fail("a tile below the limit is not covered by its prefix rows", kFenTileLimit, t, covered, i);
        checks++;
    }
    if (fen_prefix_rows(kFenTileLimit) != 0) fail("tile 16^6 was expected to be beyond the scheme", kFenTileLimit, fen_prefix_rows(kFenTileLimit), 0, 0);
    // the largest Partition that is let through, played through as well (prefixes sampled: 16.7 M tiles)
    run(kFenTileLimit - 1, false);
    std::printf("ok %lld checks\n", checks);
    return 0;
}
