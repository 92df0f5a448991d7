// lookup_image_main.cpp -- the rules for lookup images (vdl_column_image.h: use_in_aggregate, use_in_vscan, and map_range / compose
// applied to a looked-up value) against brute force over small images; built with ASan + UBSan by tests/test_lookup_images_cpu.py.
//
// A dimension table of every encoded value e the image's width holds (1 byte: all 256; 2 bytes: a band around both ends and zero),
// image[i] = e_i, column[i] = base + scale * e_i.  A fact row looks up index i.  For every range [lo, hi] out of a grid of bounds:
//   * encoded use: the row passes map_range's range on image[i]  <=>  lo <= column[i] <= hi;
//   * decoded use: img-decode(image[i]) == column[i], so the planned range applies unchanged;
//   * an aggregate factor a + s * column[i] equals compose's a' + s' * image[i] in wrapping 64-bit arithmetic;
// and the use rules say what the comments promise: a raw use of an aggregate scan admits a pure narrowing only and is never decoded,
// a per-row value of a scan with derived columns admits scale 1 only and is decoded exactly when the image is not pure.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vdl_column_image.h"

using namespace vdl::img;

static long long checks = 0;
static void fail(const char *what, const Image &im, long long a, long long b, long long c) {
    std::printf("FAIL %s: width %d base %lld scale %lld (%lld, %lld, %lld)\n", what, im.width, (long long)im.base, (long long)im.scale, a, b, c);
    std::exit(1);
}
static int64_t decode(const Image &im, int64_t e) { return (int64_t)((uint64_t)im.base + (uint64_t)im.scale * (uint64_t)e); }

int main() {
    for (int width : {1, 2}) {
        std::vector<int64_t> es;
        if (width == 1) for (int64_t e = -128; e <= 127; e++) es.push_back(e);
        else for (int64_t c : {(int64_t)-32768, (int64_t)0, (int64_t)32767}) for (int64_t d = -40; d <= 40; d++) if (c + d >= -32768 && c + d <= 32767) es.push_back(c + d);
        for (int64_t base = -3; base <= 3; base++) {
            for (int64_t scale : {(int64_t)1, (int64_t)10, (int64_t)1000}) {
                Image im;
                im.width = width; im.base = base; im.scale = scale;
                // ---- the use rules
                for (int raw = 0; raw <= 1; raw++) {
                    const Use u = use_in_aggregate(im, raw != 0);
                    const bool want = im.pure() || !raw;
                    if ((u != USE_CATALOG) != want || u == USE_DECODED) fail("use_in_aggregate", im, raw, u, 0);
                    const Use v = use_in_vscan(im, raw != 0);
                    const bool wantv = scale == 1 || !raw;
                    if ((v != USE_CATALOG) != wantv) fail("use_in_vscan", im, raw, v, 0);
                    if (wantv && (v == USE_DECODED) != (raw && !im.pure())) fail("decoded exactly when needed per row and not pure", im, raw, v, 0);
                    if (v == USE_DECODED && scale != 1) fail("a per-row decode costs an add", im, raw, v, 0);
                    checks += 4;
                }
                Image none;
                if (use_in_aggregate(none, false) != USE_CATALOG || use_in_vscan(none, false) != USE_CATALOG) fail("no image", none, 0, 0, 0);
                // ---- the dimension table and its image
                std::vector<int64_t> column, image;
                for (int64_t e : es) { image.push_back(e); column.push_back(decode(im, e)); }
                // ---- bounds: around both ends of the decoded range, around zero, the sentinels, and far outside
                std::vector<int64_t> bounds = {INT64_MIN, INT64_MIN + 1, INT64_MAX - 1, INT64_MAX};
                const int64_t vlo = decode(im, es.front()), vhi = decode(im, es.back());
                for (int64_t c : {vlo, (int64_t)0, vhi, base})
                    for (int64_t d = -2 * scale - 2; d <= 2 * scale + 2; d += (scale > 10 ? scale / 4 + 1 : 1)) bounds.push_back(c + d);
                for (int64_t lo : bounds) {
                    for (int64_t hi : bounds) {
                        int64_t elo, ehi;
                        map_range(im, lo, hi, &elo, &ehi);
                        for (size_t i = 0; i < image.size(); i++) {      // a fact row whose join index is i
                            const bool want = column[i] >= lo && column[i] <= hi;
                            const bool enc = image[i] >= elo && image[i] <= ehi;
                            if (enc != want) fail("map_range then lookup", im, lo, hi, image[i]);
                            const int64_t dec = decode(im, image[i]);
                            if ((dec >= lo && dec <= hi) != want) fail("lookup then decode", im, lo, hi, image[i]);
                            checks += 2;
                        }
                    }
                }
                // ---- aggregate factors over the looked-up value, wrapping
                for (int64_t a : {(int64_t)0, (int64_t)100, (int64_t)-7, INT64_MAX})
                    for (int64_t s : {(int64_t)1, (int64_t)-1, (int64_t)3, ((int64_t)1 << 61) + 5, INT64_MIN}) {
                        int64_t a2, s2;
                        compose(im, a, s, &a2, &s2);
                        for (size_t i = 0; i < image.size(); i++) {
                            const uint64_t want = (uint64_t)a + (uint64_t)s * (uint64_t)column[i], got = (uint64_t)a2 + (uint64_t)s2 * (uint64_t)image[i];
                            if (want != got) fail("compose then lookup", im, a, s, image[i]);
                            checks++;
                        }
                    }
            }
        }
    }
    std::printf("ok %lld checks\n", checks);
    return 0;
}
