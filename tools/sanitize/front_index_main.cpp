// front_index_main.cpp -- the look-back of the one-pass fused front (vdl_mscan_body.h: project_front_body) played through on the host
// with one count per batch, over the very index functions and the very prefix walk the kernel runs (vdl_front_index.h), 64 lanes
// modelled; built by tests/test_front_index_cpu.py: with ASan + UBSan for the smaller counts, plainly for the largest.
//
// For a number of batches:
//   * every batch u stores node (u, 0) = its own count and, for j = 1, 2, ... while 16^j divides u + 1, node (u, j) = node (u, j - 1) plus
//     the 15 nodes front_sibling(u, j, lane), lane < 15 -- the publisher loop of the kernel's first wave;
//   * the prefix of batch t is the sum over 64 lanes of front_prefix_walk(nbatches, t, lane, wait) -- the statements the kernel's last wave
//     executes, striding `i` included -- and must equal the plain sum of the counts of the batches before t;
//   * every word read or written lies in [0, front_look_words(nbatches)); no two nodes share a word; a word that is read has been stored
//     by some batch (the kernel would poll a word nobody stores for ever) and by a batch with a SMALLER number than the reader's (batches
//     take their numbers from a counter, so those are the batches known to be running); no word is read twice for one prefix.  EVERY prefix of every count is checked.
// Counts are random numbers up to 8192 x 2^20, so the sums pass 2^32 early and stay below the ready bit.
//
// A lane takes a second node of a prefix only when the hex digits of the batch number sum to more than 64: from batch 0x5FFFF on, which a
// device would need 3.2 G rows to reach.  The program counts the prefixes in which that happened and prints the number.
//
// Build with -DVDL_FRONT_BATCH=<tiles per batch of vdl_mscan_body.h>: the largest run the launcher lets through follows from it.
// usage: front_index_main [--largest-only | --no-largest]   (every prefix of every count is checked either way)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vdl_front_index.h"

#ifndef VDL_FRONT_BATCH
#error "build with -DVDL_FRONT_BATCH=<tiles per batch, as csrc/vdl_mscan_body.h defines it>"
#endif

using namespace vdl;

static long long checks = 0, second_trips = 0;
static void fail(const char *what, long long nbatches, long long a, long long b, long long c) {
    std::printf("FAIL %s: %lld batches (%lld, %lld, %lld)\n", what, nbatches, a, b, c);
    std::exit(1);
}
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

constexpr uint64_t kReady = 1ull << 63;                    // (kFrontReady of the kernel: a word nobody has stored is 0)

struct Nodes {
    int64_t nbatches, nwords;
    std::vector<uint64_t> word;          // {ready, count}, zeroed as the launcher zeroes them
    std::vector<uint32_t> owner;         // the batch that stored the word (valid where ready)
    std::vector<uint32_t> read_for;      // 1 + the batch whose prefix read the word last
    explicit Nodes(int64_t nb) : nbatches(nb), nwords(front_look_words(nb)), word((size_t)nwords, 0), owner((size_t)nwords, 0), read_for((size_t)nwords, 0) {}
    void store(int64_t u, int j, uint64_t v) {
        const int64_t w = front_node(nbatches, u, j);
        if (w < 0 || w >= nwords) fail("a node is stored outside the words", nbatches, u, j, w);
        if (word[(size_t)w] & kReady) fail("two nodes share a word", nbatches, u, j, w);
        if (v & kReady) fail("a count reaches the ready bit", nbatches, u, j, 0);
        word[(size_t)w] = v | kReady; owner[(size_t)w] = (uint32_t)u;
        checks += 3;
    }
    uint64_t load(int64_t w, int64_t reader, const char *who) const {
        if (w < 0 || w >= nwords) fail(who, nbatches, reader, w, nwords);
        if (!(word[(size_t)w] & kReady)) fail("a word is read that no batch stores (the kernel would wait for ever)", nbatches, reader, w, 0);
        if ((int64_t)owner[(size_t)w] >= reader) fail("a batch waits for a node of a batch that is not before it", nbatches, reader, w, owner[(size_t)w]);
        checks += 3;
        return word[(size_t)w] & ~kReady;
    }
};

static int digit_sum(int64_t t) { int s = 0; for (; t; t >>= kFrontFanBits) s += (int)(t & (kFrontFan - 1)); return s; }

// the prefix of EVERY batch is checked
static void run(int64_t nbatches) {
    std::vector<uint32_t> count((size_t)nbatches);
    for (auto &c : count) c = (uint32_t)(rnd() % ((8192ull << 20) + 1));
    Nodes N(nbatches);
    // ---- publication, batch by batch in ticket order: a batch reads nodes of earlier batches only, so this order finds them all stored
    int64_t nodes = 0;
    for (int64_t u = 0; u < nbatches; u++) {
        uint64_t acc = count[(size_t)u];
        N.store(u, 0, acc);
        nodes++;
        for (int j = 1; j < kFrontLevels && front_publishes(u, j); j++) {
            for (int lane = 0; lane < kFrontFan - 1; lane++) {
                const int64_t w = front_sibling(nbatches, u, j, lane);
                const int64_t sib = u - ((int64_t)(lane + 1) << (kFrontFanBits * (j - 1)));
                if (sib < 0) fail("a sibling before batch 0", nbatches, u, j, sib);
                if (w != front_node(nbatches, sib, j - 1)) fail("a sibling's word is not the node of that batch one level down", nbatches, u, j, w);
                acc += N.load(w, u, "a sibling's word lies outside the words");
            }
            N.store(u, j, acc);
            nodes++;
        }
    }
    // every word is taken, and the words are exactly as many as the nodes
    int64_t stored = 0;
    for (int64_t w = 0; w < N.nwords; w++) stored += (N.word[(size_t)w] & kReady) != 0;
    if (stored != nodes || stored != N.nwords) fail("words, nodes and stored words differ in number", nbatches, N.nwords, nodes, stored);
    // ---- the prefixes: 64 lanes, each running the kernel's walk
    uint64_t before = 0;
    for (int64_t t = 0; t < nbatches; t++) {
        {
            uint64_t sum = 0;
            int reads = 0, most = 0;
            for (int lane = 0; lane < kFrontWave; lane++) {
                int mine = 0;
                sum += (uint64_t)front_prefix_walk(nbatches, t, lane, [&](int64_t w) {
                    if (reads >= kFrontLevels * (kFrontFan - 1)) fail("more nodes in a prefix than seven levels have", nbatches, t, reads, 0);
                    const int64_t v = (int64_t)N.load(w, t, "a prefix node lies outside the words");           // (checks the index first)
                    if (N.read_for[(size_t)w] == (uint32_t)(t + 1)) fail("a node is read twice for one prefix", nbatches, t, w, lane);
                    N.read_for[(size_t)w] = (uint32_t)(t + 1);
                    reads++;
                    mine++;
                    return v;
                });
                if (mine > most) most = mine;
            }
            if (reads != digit_sum(t)) fail("a prefix is made of one node per unit of each hex digit", nbatches, t, reads, digit_sum(t));
            if (sum != before) fail("prefix", nbatches, t, (long long)sum, (long long)before);
            if ((most > 1) != (reads > kFrontWave)) fail("second trips happen exactly when the digits sum to more than 64", nbatches, t, most, reads);
            if (most > 1) second_trips++;
            checks += 3;
        }
        before += count[(size_t)t];
    }
}

int main(int argc, char **argv) {
    static_assert(kFrontFan == 16 && kFrontLevels == 7 && kFrontWave == 64, "the batch counts below are chosen for seven levels of fan-out 16 and 64 lanes");
    const bool largest_only = argc > 1 && !std::strcmp(argv[1], "--largest-only"), no_largest = argc > 1 && !std::strcmp(argv[1], "--no-largest");
    if (!largest_only)
        for (int64_t nb : {(int64_t)1, (int64_t)15, (int64_t)16, (int64_t)17, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)0x111, (int64_t)0xFFF, (int64_t)0x1000,
                           (int64_t)0x1001, (int64_t)0xFFFF, (int64_t)0x10000, (int64_t)0x10001, (int64_t)0xFFFFF, (int64_t)0x100000 + 17})
            run(nb);
    // ---- the limit.  launch_project_front refuses 16^7 TILES and more, the tree is over BATCHES of VDL_FRONT_BATCH tiles: the largest run
    // let through has ceil((16^7 - 1) / VDL_FRONT_BATCH) batches, and seven levels express batch numbers below kFrontBatchLimit = 16^7.  So the
    // limit is on the safe side by the factor VDL_FRONT_BATCH (4 as the library is built: the largest batch number, 0x3FFFFFF, has a top
    // digit of 3); that is arithmetic and the comment beside the launcher's check says it -- what is CHECKED here is that largest run itself.
    static_assert(VDL_FRONT_BATCH >= 1, "tiles per batch");
    const int64_t largest = (kFrontBatchLimit - 1 + VDL_FRONT_BATCH - 1) / VDL_FRONT_BATCH;
    if (!no_largest) run(largest);
    std::printf("largest run: %lld batches of %d tiles, below the %lld batches seven levels express by a factor of %lld\n", (long long)largest, (int)VDL_FRONT_BATCH,
                (long long)kFrontBatchLimit, (long long)(kFrontBatchLimit / largest));
    std::printf("ok %lld checks, %lld prefixes with a second trip\n", checks, second_trips);      // (the last line: the test reads it)
    return 0;
}
