// The rules of vdl_column_image.h against brute force (tests/test_column_images_cpu.py builds this under ASan + UBSan):
//   choose   -- the width is the narrowest that holds the column, the pure narrowing wins ties, every value round-trips;
//   map_range -- for every encoded value e of the width, lo <= base + scale * e <= hi  <=>  elo <= e <= ehi;
//   compose  -- a + s * (base + scale * e) == a' + s' * e in wrapping 64-bit arithmetic.
// Exit status 0 and "ok <checks>" on success; the first failure is printed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vdl_column_image.h"

using namespace vdl;

static long long checks = 0;
#define CHECK(cond, ...) do { checks++; if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static __int128 value(const img::Image &im, int64_t e) { return (__int128)im.base + (__int128)im.scale * e; }

// every e of the width when it is 1 byte; otherwise e near the ends, near the mapped bounds and a spread between
static std::vector<int64_t> probes(const img::Image &im, int64_t elo, int64_t ehi) {
    std::vector<int64_t> out;
    const int64_t wlo = img::width_min(im.width), whi = img::width_max(im.width);
    if (im.width == 1) { for (int64_t e = wlo; e <= whi; e++) out.push_back(e); return out; }
    for (int64_t c : {wlo, whi, elo, ehi, (int64_t)0})
        for (int64_t d = -3; d <= 3; d++) { const __int128 e = (__int128)c + d; if (e >= wlo && e <= whi) out.push_back((int64_t)e); }
    for (int k = 0; k <= 64; k++) out.push_back(wlo + (int64_t)(((__int128)whi - wlo) * k / 64));
    return out;
}

static void check_range(const img::Image &im, int64_t lo, int64_t hi) {
    int64_t elo = 0, ehi = 0;
    img::map_range(im, lo, hi, &elo, &ehi);
    if (lo == INT64_MIN && hi == INT64_MAX) { CHECK(elo == lo && ehi == hi, "sentinels kept"); return; }
    CHECK(elo >= img::width_min(im.width) || elo > ehi, "lower bound inside the width");
    CHECK(ehi <= img::width_max(im.width) || elo > ehi, "upper bound inside the width");
    for (int64_t e : probes(im, elo, ehi)) {
        const __int128 v = value(im, e);
        const bool want = v >= lo && v <= hi, got = e >= elo && e <= ehi;
        CHECK(want == got, "w%d base %lld scale %lld [%lld, %lld] -> [%lld, %lld]: e %lld", im.width, (long long)im.base, (long long)im.scale,
              (long long)lo, (long long)hi, (long long)elo, (long long)ehi, (long long)e);
    }
}

static void check_compose(const img::Image &im, int64_t a, int64_t s) {
    int64_t a2 = 0, s2 = 0;
    img::compose(im, a, s, &a2, &s2);
    CHECK(img::plain(a2, s2) == (a2 == 0 && s2 == 1), "plain bit");
    for (int64_t e : probes(im, 0, 0)) {
        const uint64_t v = (uint64_t)im.base + (uint64_t)im.scale * (uint64_t)e;
        CHECK((uint64_t)a + (uint64_t)s * v == (uint64_t)a2 + (uint64_t)s2 * (uint64_t)e, "compose a %lld s %lld e %lld", (long long)a, (long long)s, (long long)e);
    }
}

int main() {
    // ---- choose ----------------------------------------------------------------------------------
    struct C { int stored; int64_t mn, mx; int p; int width; int64_t base, scale; };
    const C cases[] = {
        {4, 727564, 730089, 0, 2, 727564, 1},                     // l_shipdate: (v - min) in int16
        {8, 0, 10, 0, 1, 0, 1},                                   // l_discount: a pure narrowing
        {8, 100, 5000, 2, 1, 100, 100},                           // l_quantity: (v - 100) / 100
        {8, 90091, 10494950, 0, 4, 0, 1},                         // l_extendedprice: int32 as it is
        {4, 16, 64, 0, 1, 0, 1},                                  // dictionary codes: the pure narrowing ties with the affine form and wins
        {8, -5, -5, 19, 1, 0, 1},                                 // a single value
        {8, INT64_MIN, INT64_MAX, 0, 0, 0, 1},                    // max - min overflows: none
        {4, INT32_MIN, INT32_MAX, 0, 0, 0, 1},                    // nothing narrower
        {2, -128, 127, 0, 1, 0, 1},
        {1, 0, 1, 0, 0, 0, 1},                                    // already 1 byte
        {8, -1000000000000000000ll, 1000000000000000000ll, 18, 1, -1000000000000000000ll, 1000000000000000000ll},
        {8, 5, 5 + 127 * 1000, 3, 1, 5, 1000},
        {8, 5, 5 + 128 * 1000, 3, 2, 5, 1000},                    // one past the int8 range
        // the width limits exactly, at both ends of int64
        {4, -32768, 32767, 0, 2, 0, 1},                           // int16's range stored in 4 bytes: a pure narrowing
        {8, -32769, 32767, 0, 4, 0, 1},                           // one below it
        {8, -128, 127, 0, 1, 0, 1},
        {8, -128, 128, 0, 2, 0, 1},
        {8, INT64_MAX - 3 - 2147483647ll, INT64_MAX - 3, 0, 4, INT64_MAX - 3 - 2147483647ll, 1},   // span 2^31 - 1 near INT64_MAX
        {8, INT64_MAX - 2147483647ll, INT64_MAX, 0, 4, INT64_MAX - 2147483647ll, 1},               // ... ending on it
        {8, 1ll << 40, (1ll << 40) + 2147483648ll, 0, 0, 0, 1},   // span 2^31: none
        {8, INT64_MIN, INT64_MIN + 2147483647ll, 0, 4, INT64_MIN, 1},
        {8, INT64_MIN, INT64_MIN + 2147483648ll, 0, 0, 0, 1},
        {8, INT64_MIN, INT64_MIN + 127 * 1000, 3, 1, INT64_MIN, 1000},
        {8, INT64_MIN, INT64_MIN + 128 * 1000, 3, 2, INT64_MIN, 1000},
        {8, INT64_MIN, INT64_MIN + 30000ll * 1000, 3, 2, INT64_MIN, 1000},
        {8, -(1ll << 62) + 7, -(1ll << 62) + 7 + 127 * 1000, 3, 1, -(1ll << 62) + 7, 1000},
        {8, -(1ll << 62) + 7, -(1ll << 62) + 7 + 128 * 1000, 3, 2, -(1ll << 62) + 7, 1000},
    };
    for (const C &t : cases) {
        const img::Image im = img::choose(t.stored, t.mn, t.mx, t.p);
        CHECK(im.width == t.width, "choose(%d, %lld, %lld, %d): width %d, want %d", t.stored, (long long)t.mn, (long long)t.mx, t.p, im.width, t.width);
        if (im.width) CHECK(im.base == t.base && im.scale == t.scale, "choose(%lld, %lld): base %lld scale %lld", (long long)t.mn, (long long)t.mx, (long long)im.base, (long long)im.scale);
    }
    // brute force over small domains: the image holds every multiple of the scale between min and max, the width is the narrowest
    for (int64_t mn : {(int64_t)-70000, (int64_t)-300, (int64_t)-1, (int64_t)0, (int64_t)7, (int64_t)40000, (int64_t)3000000000ll})
        for (int64_t span : {(int64_t)0, (int64_t)1, (int64_t)126, (int64_t)127, (int64_t)128, (int64_t)255, (int64_t)40000, (int64_t)70000, (int64_t)5000000000ll})
            for (int p = 0; p <= 18; p++) {
                const int64_t sc = img::pow10(p);
                if (span > INT64_MAX / sc) continue;
                const int64_t mx = mn + span * sc;
                for (int stored : {2, 4, 8}) {
                    if (img::narrowest(mn, mx) > stored) continue;          // (the column holds its values)
                    const img::Image im = img::choose(stored, mn, mx, p);
                    int best = stored;
                    for (int w : {4, 2, 1}) if (img::narrowest(mn, mx) <= w || img::narrowest(0, span) <= w) best = w;
                    CHECK(im.width == (best < stored ? best : 0), "width of [%lld, %lld] p %d stored %d: %d", (long long)mn, (long long)mx, p, stored, im.width);
                    if (!im.width) continue;
                    if (!im.pure()) CHECK(img::narrowest(mn, mx) > im.width, "the pure narrowing wins ties");
                    for (int64_t k : {(int64_t)0, (int64_t)1, span / 2, span}) {
                        if (k > span) continue;
                        const int64_t v = mn + k * sc;
                        const int64_t e = (int64_t)((uint64_t)(v - im.base) / (uint64_t)im.scale);
                        CHECK(e >= img::width_min(im.width) && e <= img::width_max(im.width) && value(im, e) == v, "round trip of %lld: [%lld, %lld] p %d stored %d -> w%d base %lld scale %lld", (long long)v, (long long)mn, (long long)mx, p, stored, im.width, (long long)im.base, (long long)im.scale);
                    }
                }
            }
    // ---- map_range and compose -------------------------------------------------------------------
    std::vector<img::Image> ims;
    for (int w : {1, 2, 4})
        for (int64_t base : {(int64_t)0, (int64_t)-7, (int64_t)727564, (int64_t)-1000000000000000000ll, (int64_t)INT64_MIN / 2})
            for (int p : {0, 1, 2, 3, 9, 17, 18}) {
                img::Image im; im.width = w; im.base = base; im.scale = img::pow10(p);
                if ((__int128)base + (__int128)im.scale * img::width_max(w) > INT64_MAX) continue;
                if ((__int128)base + (__int128)im.scale * img::width_min(w) < INT64_MIN) continue;
                ims.push_back(im);
            }
    // images that start at INT64_MIN or end at INT64_MAX (their encoded values are >= 0: the negative half of the width lies
    // outside int64 and is never stored)
    for (int w : {1, 2, 4})
        for (int p : {0, 3}) {
            img::Image lo; lo.width = w; lo.base = INT64_MIN; lo.scale = img::pow10(p);
            ims.push_back(lo);
            img::Image hi; hi.width = w; hi.scale = img::pow10(p); hi.base = (int64_t)((__int128)INT64_MAX - (__int128)hi.scale * img::width_max(w));
            ims.push_back(hi);
        }
    for (const img::Image &im : ims) {
        std::vector<int64_t> ends = {INT64_MIN, INT64_MAX, INT64_MIN + 1, INT64_MAX - 1, 0, -1, 1, im.base};
        if (im.base > INT64_MIN) ends.push_back(im.base - 1);
        if (im.base < INT64_MAX) ends.push_back(im.base + 1);
        for (int64_t e : {img::width_min(im.width), img::width_max(im.width), (int64_t)0, (int64_t)-1, (int64_t)1, (int64_t)22, (int64_t)-23}) {
            const __int128 v = value(im, e);
            for (int d : {-1, 0, 1}) { const __int128 x = v + d; if (x >= INT64_MIN && x <= INT64_MAX) ends.push_back((int64_t)x); }
            const __int128 half = v + im.scale / 2;                      // between two multiples of the scale
            if (half >= INT64_MIN && half <= INT64_MAX) ends.push_back((int64_t)half);
        }
        for (int64_t lo : ends)
            for (int64_t hi : ends) check_range(im, lo, hi);
        for (int64_t a : {(int64_t)0, (int64_t)100, (int64_t)-1, INT64_MIN, INT64_MAX})
            for (int64_t s : {(int64_t)1, (int64_t)-1, (int64_t)0, (int64_t)7, INT64_MAX, INT64_MIN}) check_compose(im, a, s);
    }
    // the Q6 filters of tests/golden/q6.vdl over the images of the l_* columns
    {
        const img::Image ship = img::choose(4, 727564, 730089, 0), qty = img::choose(8, 100, 5000, 2);
        int64_t lo, hi;
        img::map_range(ship, 728294, 728658, &lo, &hi);
        CHECK(lo == 728294 - 727564 && hi == 728658 - 727564, "shipdate range");
        img::map_range(qty, INT64_MIN, 2399, &lo, &hi);
        CHECK(lo == -128 && hi == 22, "quantity < 24.00 -> e <= 22 (v <= 2300): [%lld, %lld]", (long long)lo, (long long)hi);
        img::map_range(qty, 150, 199, &lo, &hi);
        CHECK(lo > hi, "no multiple of 100 in [150, 199]");
    }
    std::printf("ok %lld\n", checks);
    return 0;
}
