// The bit-packed image rules of vdl_column_image.h against brute force (tests/test_packed_images_cpu.py builds this under ASan + UBSan):
//   bit_length / pack -- bits is the bit length of emax - emin (1 for a constant column) for every span up to 2^32, a packed image
//                        exists exactly when bits < 8 x the byte width, and base' = base + scale * emin (wrapping);
//   map_range_packed  -- for every sub-range [lo, hi] of small domains and every stored e' in [0, 2^bits - 1]:
//                        lo <= base' + scale * e' <= hi  <=>  plo <= e' <= phi, with plo, phi inside the domain or [1, 0];
//   compose_packed    -- a + s * (base' + scale * e') == a' + s' * e' in wrapping 64-bit arithmetic;
//   packed_at         -- row i's value starts at bit (i mod 2048) / 64 * bits of lane i mod 64's stream, dword (s bits + k) 64 + l.
// Exit status 0 and "ok <checks>" on success; the first failure is printed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vdl_column_image.h"

using namespace vdl;

static long long checks = 0;
#define CHECK(cond, ...) do { checks++; if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static int brute_bits(unsigned long long span) {
    int b = 1;
    while (b < 64 && (1ull << b) <= span) b++;
    return b;
}

static void check_bits() {
    std::vector<unsigned long long> spans;
    for (unsigned long long x = 0; x <= 70000; x++) spans.push_back(x);
    for (int k = 1; k <= 32; k++)
        for (long long d = -2; d <= 2; d++) {
            const long long x = (long long)(1ull << k) + d;
            if (x >= 0 && x <= (1ll << 32)) spans.push_back((unsigned long long)x);
        }
    for (unsigned long long s : spans) {
        const int b = img::bit_length(s);
        CHECK(b == brute_bits(s), "bit_length(%llu) = %d", s, b);
        for (int w : {1, 2, 4}) {
            img::Image im;
            im.width = w; im.base = -1000003; im.scale = 7;
            const int64_t emin = w == 1 ? -5 : -77;
            const img::Packed pk = img::pack(im, emin, (int64_t)((__int128)emin + s));
            const bool want = b <= 32 && b < 8 * w;
            CHECK((pk.bits != 0) == want, "span %llu width %d: bits %d", s, w, pk.bits);
            if (want) {
                CHECK(pk.bits == b, "span %llu: bits %d, want %d", s, pk.bits, b);
                CHECK(pk.scale == im.scale && pk.base == (int64_t)((uint64_t)im.base + (uint64_t)im.scale * (uint64_t)emin), "base' of span %llu", s);
            }
        }
    }
    img::Image im;
    im.width = 2;
    CHECK(img::pack(im, 5, 5).bits == 1, "a constant column gets 1 bit");
    CHECK(img::pack(im, 6, 5).bits == 0, "no values, no packed image");
    img::Image none;
    CHECK(img::pack(none, 0, 1).bits == 0, "no byte image, no packed image");
}

static void check_ranges() {
    // small domains: every bits 1..5, bases around the int64 ends and zero, scales 1, 3, 1000; every sub-range [lo, hi] of the
    // values around the domain (one step past both ends), and the sentinels
    for (int bits = 1; bits <= 5; bits++)
        for (int64_t base : {(int64_t)0, (int64_t)-17, (int64_t)INT64_MIN, (int64_t)(INT64_MAX - 40000)})
            for (int64_t scale : {(int64_t)1, (int64_t)3, (int64_t)1000}) {
                img::Packed pk;
                pk.bits = bits; pk.base = base; pk.scale = scale;
                const int64_t top = (1ll << bits) - 1;
                std::vector<int64_t> vals;
                for (int64_t e = -2; e <= top + 2; e++)
                    for (int64_t d : {(int64_t)-1, (int64_t)0, (int64_t)1}) {
                        const __int128 v = (__int128)base + (__int128)scale * e + d;
                        if (v >= INT64_MIN && v <= INT64_MAX) vals.push_back((int64_t)v);
                    }
                vals.push_back(INT64_MIN);
                vals.push_back(INT64_MAX);
                for (int64_t lo : vals)
                    for (int64_t hi : vals) {
                        int64_t plo = 0, phi = 0;
                        img::map_range_packed(pk, lo, hi, &plo, &phi);
                        if (lo == INT64_MIN && hi == INT64_MAX) { CHECK(plo == lo && phi == hi, "sentinels kept"); continue; }
                        CHECK((plo >= 0 && phi <= top && plo <= phi) || (plo == 1 && phi == 0), "bits %d [%lld, %lld] -> [%lld, %lld]", bits, (long long)lo, (long long)hi,
                              (long long)plo, (long long)phi);
                        for (int64_t e = 0; e <= top; e++) {
                            const __int128 v = (__int128)base + (__int128)scale * e;
                            const bool want = v >= lo && v <= hi, got = e >= plo && e <= phi;
                            CHECK(want == got, "bits %d base %lld scale %lld [%lld, %lld] -> [%lld, %lld]: e' %lld", bits, (long long)base, (long long)scale,
                                  (long long)lo, (long long)hi, (long long)plo, (long long)phi, (long long)e);
                        }
                    }
            }
}

static void check_compose() {
    const int64_t probes[] = {0, 1, -1, 7, 1000, INT64_MIN, INT64_MAX, -(1ll << 62) + 7, 123456789012345ll};
    for (int64_t base : probes)
        for (int64_t scale : {(int64_t)1, (int64_t)10, (int64_t)1000, (int64_t)999999937})
            for (int64_t a : probes)
                for (int64_t s : probes) {
                    img::Packed pk;
                    pk.bits = 12; pk.base = base; pk.scale = scale;
                    int64_t a2 = 0, s2 = 0;
                    img::compose_packed(pk, a, s, &a2, &s2);
                    for (int64_t e : {(int64_t)0, (int64_t)1, (int64_t)2525, (int64_t)4095}) {
                        const uint64_t v = (uint64_t)base + (uint64_t)scale * (uint64_t)e;
                        CHECK((uint64_t)a + (uint64_t)s * v == (uint64_t)a2 + (uint64_t)s2 * (uint64_t)e, "compose base %lld scale %lld a %lld s %lld e %lld",
                              (long long)base, (long long)scale, (long long)a, (long long)s, (long long)e);
                    }
                }
}

static void check_layout() {
    for (int bits = 1; bits <= 32; bits++) {
        CHECK(img::packed_dwords(1, bits) == 64 * bits, "one row: one stripe");
        CHECK(img::packed_dwords(2048, bits) == 64 * bits && img::packed_dwords(2049, bits) == 128 * bits, "whole stripes");
        for (int64_t i : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)64, (int64_t)2047, (int64_t)2048, (int64_t)4095, (int64_t)(37 * 2048 + 1999)}) {
            int64_t dw = 0;
            int bit = 0;
            img::packed_at(i, bits, &dw, &bit);
            const int64_t s = i / 2048, j = (i % 2048) / 64, l = i % 64;
            CHECK(dw == (s * bits + (j * bits) / 32) * 64 + l && bit == (int)((j * bits) % 32), "row %lld bits %d", (long long)i, bits);
            CHECK(dw < img::packed_dwords(i + 1, bits), "inside the image");
        }
    }
}

int main() {
    check_bits();
    check_ranges();
    check_compose();
    check_layout();
    std::printf("ok %lld\n", checks);
    return 0;
}
