// vdl_group_fold.inc -- the text of the kernel that runs every fold of one GROUP BY in one launch, for gfx950.  Included INTO the two
// kernels that run it: k_group_fold<NF> (vdl_ops.hip, WIDE = false) and k_wide_group_fold<NF> (vdl_fold_wide.hip, WIDE = true), which
// provide, besides the kernel's parameters vec16, heads, m and offsets:
//     NF                          folds handled per trip (the kernel's template parameter)
//     constexpr bool WIDE         a FoldSum member may have a second sum (DESIGN.md section 5.17 "The tail")
//     const GroupFoldArgs &a      the argument block, in the kernel's own parameter
//     int64_t *const *out_hi      WIDE: per member, where the sum of the high halves goes, or null; not read otherwise
// Text and no function template like the folds of vdl_fold_body.h, because the argument block must stay the kernel's parameter: behind
// a call -- an inlined one too -- the compiler unrolls the trips first and then promotes the whole block to registers at the kernel's
// entry: 16 members' kinds, sources and outputs, 400 scalar registers spilled to vector lanes, and k_group_fold<2> at 73 VGPRs and six
// waves per SIMD where this text keeps it at seven.  Read in place, every member's words are scalar loads next to their use.
//
// (the tail of a plan whose front is fused: Partition -> Scatter x k -> Fold x k over the survivors, Vlite.hs:1056-1060,1082-1098.
// Statement by statement that is a head pass, a count, a compaction per FoldChoose and fill + segmented fold + compaction per
// aggregate -- a dozen launches of a few microseconds of work each; here: one pass over the entries for all of them.)
// A block owns one compaction tile (64 head words = 4096 entries), a wave walks words of it, lane l holds entry 64 w + l.  Group of
// an entry = heads before the tile (offsets) + heads before its word inside the tile + heads at or before its lane - 1.  Values are
// folded along the lanes with a segmented shuffle scan bounded by the head word; the last lane of a segment hands the partial to
// out[group]: a plain store when the run begins and ends inside the word (nobody else adds to it), an atomic otherwise.
// Layout: a lane owns kGroupK = 8 CONSECUTIVE entries and folds them serially (no cross-lane traffic inside its chunk: a run that
// begins and ends there is stored at once); only what is open at the chunk's ends is combined across the lanes -- one segmented
// shuffle scan per 512 entries and fold, where a lane-per-entry layout paid one per 64 (that version was instruction-bound at
// 1.5 TB/s: 200 us for two folds over 18 M entries).  A wave covers 8 head words, a block half a compaction tile.
// NF = folds handled per trip (their loads are issued together).  vec16 bit f: fold f's data is int64 at a 16-byte aligned
// address -- four 16-byte loads per lane instead of eight scalar ones.
// The results of the runs that END inside a wave -- all but the wave's last one -- are staged in LDS at their group's place and stored by
// consecutive lanes (round 4): a lane storing its own groups put 64 isolated 8-byte writes into every store instruction, nine of them per
// fold and 512 entries, and the stores were 290 of the kernel's 506 us for Q3's 32 M survivors at SF100 (an ablation build without them:
// 216 us; -DVDL_GF_ABLATE=1 still builds it).
// WIDE: a FoldSum member with out_hi[j] set folds its chunk twice out of the registers one load filled -- the terms into out, their high
// halves into out_hi.  The LDS stage stays one word per group and 16 KiB: it is RUN TWICE for such a member (the second sum's groups
// pass through it after the first's have been stored), because a doubled stage of 32 KiB would halve the blocks per CU for every
// member of the launch, wide or not, while the second pass costs one more sweep of stores the member needs anyway.
#if defined(VDL_GF_ABLATE) && VDL_GF_ABLATE == 1
#define GF_STORE(g, v) do { if ((g) == -12345) stage[wave][0] = (v); } while (0)
#else
#define GF_STORE(g, v) do { stage[wave][(g) - Bw] = (v); } while (0)
#endif
    __shared__ int wprefix[kCompactWords];
    __shared__ uint64_t wmask[kCompactWords];
    __shared__ int64_t stage[256 / kWave][kWave * kGroupK];               // per wave: the results of its groups, by group
    constexpr int K = kGroupK, NW = 256 / kWave, WW = kWave * K / 64;          // WW = head words per wave (8)
    static_assert(kCompactWords == kGroupSplit * NW * WW, "a block's waves cover its share of the tile");
    const int64_t nw = (m + 63) >> 6;
    const int64_t tile = blockIdx.x / kGroupSplit;
    const int part = blockIdx.x % kGroupSplit;
    const int64_t w0 = tile * kCompactWords;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    if (tid < kCompactWords) {
        const int64_t w = w0 + tid;
        const uint64_t hm = w < nw ? heads[w] : 0ull;             // (bits past m are clear: launch_sorted_heads / k_seg_heads)
        wmask[tid] = hm;
        const int cnt = __popcll(hm);
        int incl = cnt;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) { const int y = __shfl_up(incl, off, kWave); if (lane >= off) incl += y; }
        wprefix[tid] = incl - cnt;
    }
    __syncthreads();
    const int wfirst = part * (NW * WW) + wave * WW;              // this wave's first word inside the tile
    if (((w0 + wfirst) << 6) >= m) return;                         // wave-uniform; no barrier below
    const int64_t e0 = ((w0 + wfirst) << 6) + (int64_t)lane * K;   // my first entry
    const int nv = m - e0 >= K ? K : (m - e0 > 0 ? (int)(m - e0) : 0);      // my entries inside the vector
    const unsigned hb = (unsigned)(wmask[wfirst + (lane >> 3)] >> ((lane & 7) * 8)) & 0xffu;     // their head bits
    const int c = __popc(hb);
    int incl = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) { const int y = __shfl_up(incl, off, kWave); if (lane >= off) incl += y; }
    const int64_t B = offsets[tile] + wprefix[wfirst] + (incl - c);           // run heads strictly before my first entry
    const int64_t Bw = offsets[tile] + wprefix[wfirst];                       // ... before the wave's: its first group's number
    const int ngw = __shfl(incl, kWave - 1, kWave);                           // run heads inside the wave
    const uint64_t headlanes = __ballot(c != 0);
    const uint64_t below = (1ull << lane) - 1;
    // lanes whose open end my chunk continues: a segment of lanes starts behind every lane that holds a head
    const uint64_t starts = (headlanes << 1) | 1ull;
    const int seg0 = 63 - __clzll((long long)(starts & (below | (1ull << lane))));
    const bool first_head_lane = c != 0 && (headlanes & below) == 0;
    const uint64_t later = lane == kWave - 1 ? 0ull : headlanes >> (lane + 1);
    const int next_head = later ? lane + __ffsll((long long)later) : -1;      // the next lane that holds a head
    const int fetch_from = next_head >= 0 ? next_head : kWave - 1;
    auto flush = [&](int64_t *out, int groups) {                   // the groups staged by this wave, stored by consecutive lanes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
        for (int k = lane; k < groups; k += kWave) out[Bw + k] = stage[wave][k];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();      // (the area is the next fold's)
    };
#pragma unroll
    for (int j0 = 0; j0 < kMaxGroupFolds; j0 += NF) {          // (constant indices into the argument block: scalar loads, no scratch copy)
        if (j0 >= a.nfold) break;                              // wave-uniform
        int64_t x[NF][K];
#pragma unroll
        for (int f = 0; f < NF; f++) {
            if (j0 + f >= a.nfold) break;
            const Src d = a.data[j0 + f];
            if (a.kind[j0 + f] == 3) {
#pragma unroll
                for (int j = 0; j < K; j++) x[f][j] = 1;
            } else if (((vec16 >> (j0 + f)) & 1u) && nv == K) {
                const ll2 *q = (const ll2 *)((const int64_t *)d.p + e0);
#pragma unroll
                for (int j = 0; j < K; j += 2) { const ll2 t = q[j >> 1]; x[f][j] = t.x; x[f][j + 1] = t.y; }
            } else {
#pragma unroll
                for (int j = 0; j < K; j++) x[f][j] = ld(d, j < nv ? e0 + j : (e0 < m ? e0 : 0));
            }
        }
#pragma unroll
        for (int f = 0; f < NF; f++) {
            if (j0 + f >= a.nfold) break;
            const int kind = a.kind[j0 + f];
            int64_t *out = a.out[j0 + f];
            if (kind == 4) {                                   // FoldChoose: the first value of every run
                int64_t g = B - 1;
#pragma unroll
                for (int j = 0; j < K; j++)
                    if ((hb >> j) & 1u) { g++; GF_STORE(g, x[f][j]); }
                flush(out, ngw);
                continue;
            }
            const int rk = kind == 1 ? R_MIN : kind == 2 ? R_MAX : R_SUM;
            const int passes = WIDE && kind == 0 && out_hi[j0 + f] ? 2 : 1;       // wave-uniform; the constant 1 without WIDE
            for (int pass = 0; pass < passes; pass++) {
                if (WIDE && pass) {                            // the second sum, out of the same registers
                    out = out_hi[j0 + f];
#pragma unroll
                    for (int j = 0; j < K; j++) x[f][j] >>= 32;
                }
                by_reduction(rk, [&](auto rc) {
                    constexpr int R = decltype(rc)::value;
                    int64_t acc = r_identity(R), pre = r_identity(R), g = B - 1;
                    bool started = false;
#pragma unroll
                    for (int j = 0; j < K; j++) {
                        if ((hb >> j) & 1u) {                      // (a head is always inside the vector)
                            if (started) GF_STORE(g, acc); else pre = acc;          // a run that began and ended in my chunk: stored at once
                            g++; acc = x[f][j]; started = true;
                        } else if (j < nv) {
                            acc = r_combine(R, acc, x[f][j]);
                        }
                    }
                    const int64_t tail = started ? acc : r_identity(R);         // open at my chunk's end (group g)
                    int64_t S = started ? pre : acc;                            // continues what was open before my chunk (group B - 1)
#pragma unroll
                    for (int off = 1; off < kWave; off <<= 1) {
                        const int64_t y = __shfl_up(S, off, kWave);
                        if (lane - off >= seg0) S = r_combine(R, S, y);
                    }
                    // S of a lane with a head (or of lane 63) = everything between the previous head lane and this lane's first head
                    const int64_t cont = __shfl(S, fetch_from, kWave);
                    if (c != 0) {
                        if (next_head >= 0) GF_STORE(g, r_combine(R, tail, cont));                                  // the run ends inside the wave
                        else atomic_combine(R, &out[g], lane == kWave - 1 ? tail : r_combine(R, tail, cont));    // it may go on in the next wave
                        if (first_head_lane && B > 0) atomic_combine(R, &out[B - 1], S);                         // ... and this one came from an earlier wave
                    } else if (headlanes == 0 && lane == kWave - 1 && B > 0) {
                        atomic_combine(R, &out[B - 1], S);                                                       // a wave inside one long run
                    }
                });
                // every group but the wave's last one has ended inside the wave and lies in the staging area: consecutive lanes store them
                flush(out, ngw - 1);
            }
        }
    }
#undef GF_STORE
