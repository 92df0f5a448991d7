// vdl_front_index.h -- the index arithmetic of the one-pass fused front's look-back (vdl_mscan_body.h: project_front_body): which word
// holds which node of the fan-out-16 Fenwick tree over the BATCHES of tiles, which batch publishes which level and from which 15 nodes,
// and the walk in which the 64 lanes of a wave collect the nodes of a batch's prefix.  Pure functions of the batch numbers, shared by the
// kernels -- precompiled and specialised: this text is part of what hiprtc compiles (csrc/Makefile, vdl_jit_src.inc), so HIP built-ins
// only -- and by a host program that plays the protocol through for batch counts no device test reaches
// (tools/sanitize/front_index_main.cpp, built with ASan + UBSan by tests/test_front_index_cpu.py).
#pragma once
#if !defined(__HIPCC_RTC__)
#include <cstdint>
#endif

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define VDL_FRONT_INDEX_FN __device__ __forceinline__
#define VDL_FRONT_INDEX_HOST_FN __host__ __device__ inline
#else
#define VDL_FRONT_INDEX_FN static inline
#define VDL_FRONT_INDEX_HOST_FN static inline
#endif

namespace vdl {

constexpr int kFrontFanBits = 4, kFrontFan = 1 << kFrontFanBits, kFrontLevels = 7;         // batches < 16^7
constexpr int kFrontWave = 64;                             // lanes that share a prefix walk (the kernels assert it is their wave)
// Batch numbers below 16^7 are the sum of the units of their seven hex digits, which is what a prefix is made of; batch 16^7 would be
// the first whose prefix the nodes cannot express (all seven digits zero, though batches come before it).
constexpr int64_t kFrontBatchLimit = (int64_t)1 << (kFrontFanBits * kFrontLevels);

// word of node (u, level) among a run's nodes: level j holds the batches u with 16^j | u + 1, in order
VDL_FRONT_INDEX_HOST_FN int64_t front_look_words(int64_t nbatches) { int64_t w = 0; for (int j = 0; j < kFrontLevels; j++) w += nbatches >> (kFrontFanBits * j); return w; }
VDL_FRONT_INDEX_FN int64_t front_node(int64_t nbatches, int64_t u, int level) {
    int64_t base = 0;
    for (int j = 0; j < level; j++) base += nbatches >> (kFrontFanBits * j);
    return base + ((u + 1) >> (kFrontFanBits * level)) - 1;
}
// batch u makes the node of level j (the count of the 16^j batches that end at u) iff 16^j divides u + 1 ...  (project_front_body spells
// this expression out in its loop over the levels: behind a call one constant of the kernel came out in another form.)
VDL_FRONT_INDEX_FN bool front_publishes(int64_t u, int level) { return ((u + 1) & (((int64_t)1 << (kFrontFanBits * level)) - 1)) == 0; }
// ... as its own node of level j - 1 plus the 15 nodes of that level before it: lane i < 15 fetches this one
VDL_FRONT_INDEX_FN int64_t front_sibling(int64_t nbatches, int64_t u, int level, int i) {
    const int64_t step = (int64_t)1 << (kFrontFanBits * (level - 1));
    return front_node(nbatches, u - (int64_t)(i + 1) * step, level - 1);
}
// The prefix walk of one lane: the nodes of batch's prefix -- one per unit of each hex digit of the batch number, level by level -- are
// dealt to the lanes in turn, node g of the concatenated list to lane g % 64; `WAIT(word)` is the count of the node in that word and
// `x` receives the lane's share of the prefix.  (Up to 7 x 15 = 105 nodes: a lane takes a second node only when the digits sum to more
// than 64.)  These statements are a macro and not a function because the kernel must run this very text and, behind a call -- a lambda
// or a functor, inlining forced -- the compiler allocated the front's registers differently (profiles/r20/README.md).
#define VDL_FRONT_PREFIX_WALK(x, nbatches, batch, lane, WAIT)                                                                              \
    do {                                                                                                                                  \
        int i = (lane);                                                                                                                   \
        for (int j = 0; j < kFrontLevels; j++) {                                                                                          \
            const int dgt = (int)(((batch) >> (kFrontFanBits * j)) & (kFrontFan - 1));                                                    \
            const int64_t hi = (batch) & ~(((int64_t)kFrontFan << (kFrontFanBits * j)) - 1);                                              \
            for (; i < dgt; i += kFrontWave) x += WAIT(front_node((nbatches), hi + ((int64_t)(i + 1) << (kFrontFanBits * j)) - 1, j));    \
            i -= dgt;                                  /* (lanes beyond this level's nodes move on to the next level's) */               \
        }                                                                                                                                 \
    } while (0)
#if !defined(__HIPCC__) && !defined(__HIPCC_RTC__)
// (for the host program: the same statements over a callable)
template <typename Wait>
static inline int64_t front_prefix_walk(int64_t nbatches, int64_t batch, int lane, Wait wait) {
    int64_t x = 0;
    VDL_FRONT_PREFIX_WALK(x, nbatches, batch, lane, wait);
    return x;
}
#endif

}  // namespace vdl
