// vdl_fold_global.inc -- the text of the first step of the global (single-run) fold for gfx950: per-block partials {value, first control
// slot, count}, in a wide fold four words with the sum of the high halves fourth.  Included INTO the two kernels that run it,
// k_fold_global (vdl_ops.hip, WIDE = false) and k_wide_fold_global (vdl_fold_wide.hip, WIDE = true, kind = 0), which provide
// `constexpr bool WIDE` and `kind` besides the parameters d, vd, vc, n and scratch.  Text and no function template like the finish step
// and the segmented fold in vdl_fold_body.h: as an inlined function the plain kernel came out with its wave-uniform branches turned
// into 481 more s_cselect_b32 and 5 % slower on the MI355X (100 -> 105 us over 60 M rows, profiles/r23/fold_body_bench.txt); included,
// its instruction mix is the one it had.
    constexpr int U = 8;                                        // 4 KB of data per wave in flight: a cold stream needs it
    constexpr int W = WIDE ? 4 : 3;                             // words per block in the scratch
    const int rk = kind == 1 ? R_MIN : kind == 2 ? R_MAX : R_SUM;
    const int ak = kind == 4 ? R_MIN : rk;
    const int64_t nw = (n + 63) >> 6;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t wstride = (int64_t)gridDim.x * (blockDim.x / kWave) * U;
    // per lane: the fold of its data; per wave (kept uniform, lane 0 reports them): first control slot, number of data
    // slots, and for count / choose the result itself -- all three come from the bitmap words, not from the rows
    int64_t acc = r_identity(rk);
    [[maybe_unused]] int64_t acch = 0;
    int64_t first = INT64_MAX, cnt = 0, chosen = INT64_MAX;
    by_kind(d.kind, [&](auto kd) { by_reduction(rk, [&](auto rc) {
        constexpr int RK = decltype(rc)::value;
        for (int64_t w0 = wave_index() * U; w0 < nw; w0 += wstride) {
            int64_t x[U];
            uint64_t mc[U], md[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int64_t w = w0 + u < nw ? w0 + u : nw - 1;
                const int64_t i = (w << 6) + lane;
                x[u] = kind < 3 ? ldk_stream<decltype(kd)::value>(d, i < n ? i : 0) : 0;     // wave-uniform test; masked lanes read slot 0
                const int64_t rem = n - (w << 6);
                mc[u] = w0 + u < nw ? (rem < 64 ? (1ull << rem) - 1 : ~0ull) : 0ull;
            }
            if (vc) {
                uint64_t t[U];
#pragma unroll
                for (int u = 0; u < U; u++) t[u] = vc[w0 + u < nw ? w0 + u : nw - 1];
#pragma unroll
                for (int u = 0; u < U; u++) mc[u] &= t[u];
            }
#pragma unroll
            for (int u = 0; u < U; u++) md[u] = mc[u];
            if (vd) {
                uint64_t t[U];
#pragma unroll
                for (int u = 0; u < U; u++) t[u] = vd[w0 + u < nw ? w0 + u : nw - 1];
#pragma unroll
                for (int u = 0; u < U; u++) md[u] &= t[u];
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int64_t wbase = (w0 + u) << 6;
                if (mc[u] && first == INT64_MAX) first = wbase + __ffsll((long long)mc[u]) - 1;      // words come in ascending order per wave
                if (md[u] && chosen == INT64_MAX) chosen = wbase + __ffsll((long long)md[u]) - 1;
                cnt += __popcll(md[u]);
                if ((md[u] >> lane) & 1ull) {
                    acc = r_combine(RK, acc, x[u]);
                    if constexpr (WIDE) acch += x[u] >> 32;                                          // one load, both sums
                }
            }
        }
    }); });
    if (kind == 3) acc = lane == 0 ? cnt : 0;
    else if (kind == 4) acc = lane == 0 ? chosen : INT64_MAX;
    if (lane != 0) { first = INT64_MAX; cnt = 0; }
    __shared__ int64_t red[W][256 / kWave];
    acc = wave_reduce(acc, ak); first = wave_reduce(first, R_MIN); cnt = wave_reduce(cnt, R_SUM);
    if constexpr (WIDE) acch = wave_reduce(acch, R_SUM);
    if (lane == 0) {
        red[0][wave] = acc; red[1][wave] = first; red[2][wave] = cnt;
        if constexpr (WIDE) red[3][wave] = acch;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 256 / kWave; w++) {
            acc = r_combine(ak, acc, red[0][w]); first = r_combine(R_MIN, first, red[1][w]); cnt += red[2][w];
            if constexpr (WIDE) acch += red[3][w];
        }
        scratch[W * (int64_t)blockIdx.x + 0] = acc;
        scratch[W * (int64_t)blockIdx.x + 1] = first;
        scratch[W * (int64_t)blockIdx.x + 2] = cnt;
        if constexpr (WIDE) scratch[W * (int64_t)blockIdx.x + 3] = acch;
    }
